"""What the four fuse entry points and the three sparse entry points refuse, and in which order: return code and icd_last_error
text of every bad call, through the raw library (the binding's own checks would intercept most of them). The strings are the
source's, written out; a call with two defects pins which check comes first. After the refusals one good call per entry point
must succeed: no refusal left a lock held or a staging half filled.

One index of 257 x 768 rows (max_nq 16, max_k 8), one fusion of 8 sub-lists, one grouping of 8 queries, one sparse index over 5
terms (max_nq 4, max_k 8). Three more handles exist only because a message cannot be reached without them: a fusion of 32
sub-lists (the index's and the grouping's batch bounds lie behind the fusion's), a grouping of 2 queries that is never paired
(the grouping's bound lies behind the sparse index's, and the unpaired refusal needs an unpaired grouping) and a second index
with a fusion, grouping and sparse index of its own (handles of another index)."""
import types

import numpy as np
import pytest

from rag_project_icd10_amd import _native
from test_sparse_search_gpu import make_rows

pytestmark = pytest.mark.gpu

N, DIM, VOCAB = 257, 768, 5
RRF, WEIGHTED = 0, 1
INVALID, STATE = -1, -5
FUSE = ("hybrid", "hybrid_grouped", "fuse", "fuse_grouped")
SPARSE = ("sparse", "sparse_range", "sparse_grouped")
GROUPED = ("hybrid_grouped", "fuse_grouped", "sparse_grouped")


def ptr(a):
    return None if a is None else a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data


@pytest.fixture(scope="module")
def world():
    rng = np.random.default_rng(5)
    corpus = rng.standard_normal((N, DIM), dtype=np.float32)
    corpus /= np.linalg.norm(corpus, axis=1, keepdims=True)
    levels = rng.integers(1, 4, N).astype(np.int32)
    group_of = (np.arange(N) % 19).astype(np.int32)
    rows = make_rows(N, VOCAB, 3)
    w = types.SimpleNamespace(lib=_native.load_library(), corpus=corpus)
    w.index = _native.IcdIndex(corpus, levels, device=0, max_nq=16, max_k=8, probe=False)
    w.fusion, w.fusion32 = w.index.fusion(8), w.index.fusion(32)
    w.grouping, w.unpaired = w.index.grouping(group_of, max_nq=8), w.index.grouping(group_of, max_nq=2)
    w.sp = w.index.sparse(*rows, VOCAB, max_nq=4, max_k=8)
    w.grouping.pair_sparse(w.index, w.sp)
    w.other = _native.IcdIndex(corpus[:64], levels[:64], device=0, max_nq=16, max_k=8, probe=False)
    w.o_fusion, w.o_grouping = w.other.fusion(8), w.other.grouping(group_of[:64], max_nq=8)
    w.o_sp = w.other.sparse(*make_rows(64, VOCAB, 3), VOCAB, max_nq=4, max_k=8)
    yield w
    for x in (w.o_sp, w.o_grouping, w.o_fusion, w.other, w.sp, w.unpaired, w.grouping, w.fusion32, w.fusion, w.index):
        x.close()


def call(w, entry, **kw):
    """One raw call of `entry` with host queries and host outputs: a good call unless `kw` says otherwise. Returns (rc, text)."""
    import torch
    a = dict(fusion=w.fusion, grouping=w.grouping, sp=w.sp, nq=2, R=2, limits=(4, 4), lmax=4, ranker=RRF, rrf_c=60.0, weights=None, norm=0,
             k=2 if entry in GROUPED else 4, gs=2, outs=True, qdev=0, off=True, terms=(0, 0, 3), null_terms=False)
    a.update(kw)
    nq, R, k, gs = a["nq"], a["R"], a["k"], a["gs"]
    slots = 16 * 128
    adj, fused = np.empty(slots, np.float64), np.empty(slots, np.float64)
    raw, ids, lv = np.empty(slots, np.float32), np.empty(slots, np.int64), np.empty(slots, np.int32)
    bits, grp = np.empty(slots, np.uint32), np.empty(slots, np.int32)
    if not a["outs"]:
        adj = fused = raw = ids = None
    lim = None if a["limits"] is None else np.asarray(a["limits"], np.int32)
    wts = None if a["weights"] is None else np.asarray(a["weights"], np.float64)
    h, f, g, sp = w.index._h, a["fusion"]._h, a["grouping"]._h, a["sp"]._h
    rank = (a["ranker"], a["rrf_c"], ptr(wts), a["norm"])
    lib = w.lib
    if entry in ("hybrid", "hybrid_grouped"):
        q = np.ascontiguousarray(w.corpus[:max(nq * R, 1)])
        if entry == "hybrid":
            rc = lib.icd_index_search_hybrid(h, f, ptr(q), nq, R, 0, ptr(lim), None, None, None, 0, _native.MODE_EXACT, *rank, k, 1,
                                             ptr(adj), ptr(fused), ptr(ids), ptr(lv), ptr(bits), 0, None)
        else:
            rc = lib.icd_index_search_hybrid_grouped(h, f, g, ptr(q), nq, R, 0, ptr(lim), None, None, None, *rank, k, gs, 1,
                                                     ptr(adj), ptr(fused), ptr(ids), ptr(lv), ptr(bits), ptr(grp), 0, None)
    elif entry in ("fuse", "fuse_grouped"):
        shape = (max(nq, 1), max(R, 1), max(a["lmax"], 1))
        sc = torch.linspace(1.0, 0.0, int(np.prod(shape)), device="cuda").reshape(shape).contiguous()   # (best first in every list)
        li = (torch.arange(int(np.prod(shape)), device="cuda", dtype=torch.int64) % N).reshape(shape).contiguous()
        stream = _native._current_stream_ptr(0)
        if entry == "fuse":
            rc = lib.icd_fusion_fuse_lists(h, f, ptr(sc), ptr(li), nq, R, a["lmax"], ptr(lim), *rank, k, 1,
                                           ptr(adj), ptr(fused), ptr(ids), ptr(lv), ptr(bits), 0, stream)
        else:
            rc = lib.icd_fusion_fuse_lists_grouped(h, f, g, ptr(sc), ptr(li), nq, R, a["lmax"], ptr(lim), *rank, k, gs, 1,
                                                   ptr(adj), ptr(fused), ptr(ids), ptr(lv), ptr(bits), ptr(grp), 0, stream)
    else:
        # nq queries of one term each, cycling through a["terms"] (host form); the device form's pointers are never followed by a refusal
        off = np.arange(max(nq, 0) + 1, dtype=np.int64)
        tr = np.asarray([a["terms"][i % len(a["terms"])] for i in range(max(nq, 1))], np.uint32)
        vl = np.ones(max(nq, 1), np.float32)
        if a["qdev"]:
            off, tr, vl = torch.from_numpy(off).cuda(), torch.from_numpy(tr.view(np.int32)).cuda(), torch.from_numpy(vl).cuda()
        qs = (ptr(off) if a["off"] else None, None if a["null_terms"] else ptr(tr), None if a["null_terms"] else ptr(vl), nq, k)
        if entry == "sparse":
            rc = lib.icd_sparse_search(h, sp, *qs, a["qdev"], None, 1, ptr(adj), ptr(raw), ptr(ids), ptr(lv), 0, None)
        elif entry == "sparse_range":
            radius = np.full(max(nq, 1), -1e30, np.float32)
            rc = lib.icd_sparse_search_range(h, sp, *qs, a["qdev"], None, ptr(radius), None, None, None, 0, 1,
                                             ptr(adj), ptr(raw), ptr(ids), ptr(lv), 0, None)
        else:
            rc = lib.icd_sparse_search_grouped(h, sp, g, *qs, gs, a["qdev"], None, 1, ptr(adj), ptr(raw), ptr(ids), ptr(lv), ptr(grp), 0, None)
    return rc, (lib.icd_last_error() or b"").decode()


R_MSG = "R=%d: a hybrid search takes 1 .. 8 requests per query"
K_HYBRID = "k=0: a hybrid search returns 1 .. 128 hits per query"
K_GROUPED = "k=0 group_size=2: need k >= 1, group_size >= 1 and k * group_size <= 128"
K_SPARSE = "k=0: a sparse search returns 1 .. 128 hits per query"
LMAX_MSG = "lmax=%d: a list holds 1 .. 128 hits"
OUT_NULL = "output pointer is NULL"
FUSION_OTHER, GROUPING_OTHER, SPARSE_OTHER = ("the %s was created for another index" % x for x in ("fusion", "grouping", "sparse index"))
UNPAIRED = "the grouping was never paired with a sparse index (icd_grouping_pair_sparse)"


def fuse_table(w, entry):
    grouped, lists = entry in GROUPED, entry in ("fuse", "fuse_grouped")
    k_msg = K_GROUPED if grouped else K_HYBRID
    if grouped:
        lim0, lim_over, over = "limits[0]=0 group_size=2: a request returns 1 .. 128 / group_size groups", \
            "limits[1]=65 group_size=2: a request returns 1 .. 128 / group_size groups", 65
    elif lists:
        lim0, lim_over, over = "limits[0]=0: a request returns 1 .. lmax=4 hits", "limits[1]=5: a request returns 1 .. lmax=4 hits", 5
    else:
        lim0, lim_over, over = "limits[0]=0: a request returns 1 .. 128 hits", "limits[1]=129: a request returns 1 .. 128 hits", 129
    t = [
        (dict(fusion=w.o_fusion), INVALID, FUSION_OTHER),
        (dict(R=0, limits=()), INVALID, R_MSG % 0),
        (dict(R=9, limits=(4,) * 9), INVALID, R_MSG % 9),
        (dict(k=0), INVALID, k_msg),
        (dict(limits=None), INVALID, "limits is NULL"),
        (dict(limits=(0, 4)), INVALID, lim0),
        (dict(limits=(4, over)), INVALID, lim_over),
        (dict(nq=5), INVALID, "nq * R = 10 exceeds the fusion's max_total=8"),
        (dict(rrf_c=0.0), INVALID, "rrf_c=0: need 0 < c < 16384"),
        (dict(rrf_c=16384.0), INVALID, "rrf_c=16384: need 0 < c < 16384"),
        (dict(ranker=WEIGHTED), INVALID, "weights is NULL"),
        (dict(ranker=WEIGHTED, weights=(-0.1, 0.5)), INVALID, "weights[0]=-0.1: a weight lies in [0, 1]"),
        (dict(ranker=WEIGHTED, weights=(0.5, np.nan)), INVALID, "weights[1]=nan: a weight lies in [0, 1]"),
        (dict(ranker=WEIGHTED, weights=(0.5, 0.5), norm=7), INVALID, "norm=7"),
        (dict(ranker=9), INVALID, "ranker=9"),
        (dict(outs=False), INVALID, OUT_NULL),
        # two defects: the earlier check wins
        (dict(R=9, limits=(4,) * 9, k=0), INVALID, R_MSG % 9),
        (dict(k=0, limits=(0, 4)), INVALID, k_msg),
        (dict(nq=5, ranker=9), INVALID, "nq * R = 10 exceeds the fusion's max_total=8"),
        (dict(rrf_c=0.0, outs=False), INVALID, "rrf_c=0: need 0 < c < 16384"),
        (dict(ranker=WEIGHTED, weights=(0.5, 2.0), norm=7), INVALID, "weights[1]=2: a weight lies in [0, 1]"),
    ]
    if entry == "hybrid":
        t += [(dict(limits=(4, 9)), INVALID, "limit 9 exceeds the index's max_k=8"),
              (dict(fusion=w.fusion32, nq=9), INVALID, "nq * R = 18 exceeds the index's max_nq=16"),
              (dict(fusion=w.fusion32, nq=9, ranker=9), INVALID, "nq * R = 18 exceeds the index's max_nq=16")]
    if grouped:
        t += [(dict(grouping=w.o_grouping), INVALID, GROUPING_OTHER),
              (dict(fusion=w.o_fusion, grouping=w.o_grouping), INVALID, FUSION_OTHER),
              (dict(fusion=w.fusion32, nq=5), INVALID, "nq * R = 10 exceeds the grouping's max_nq=8"),
              (dict(fusion=w.fusion32, nq=5, rrf_c=0.0), INVALID, "nq * R = 10 exceeds the grouping's max_nq=8")]
    if lists:
        # the grouped form checks lmax behind everything the two grouped entry points share, the plain form in front of the limits
        t += [(dict(lmax=0), INVALID, LMAX_MSG % 0), (dict(lmax=129), INVALID, LMAX_MSG % 129),
              (dict(lmax=0, k=0), INVALID, k_msg),
              (dict(lmax=0, ranker=9), INVALID, "ranker=9" if grouped else LMAX_MSG % 0)]
    return t


def sparse_table(w, entry):
    grouped = entry == "sparse_grouped"
    k_msg = K_GROUPED if grouped else K_SPARSE
    t = [
        (dict(sp=w.o_sp), INVALID, SPARSE_OTHER),
        (dict(k=0), INVALID, k_msg),
        (dict(nq=5), INVALID, "nq=5 exceeds the sparse index's max_nq=4"),
        (dict(outs=False), INVALID, OUT_NULL),
        (dict(off=False), INVALID, "q_off is NULL"),
        (dict(terms=(0, 7)), INVALID, "query 1: term 7 outside the vocabulary's [0, 5)"),
        (dict(qdev=1, null_terms=True), INVALID, "q_terms / q_vals NULL"),
        # two defects: the earlier check wins
        (dict(k=0, nq=5), INVALID, k_msg),
        (dict(nq=5, outs=False), INVALID, "nq=5 exceeds the sparse index's max_nq=4"),
        (dict(outs=False, off=False), INVALID, OUT_NULL),
    ]
    if grouped:
        t += [(dict(grouping=w.o_grouping), INVALID, GROUPING_OTHER),
              (dict(sp=w.o_sp, grouping=w.o_grouping), INVALID, SPARSE_OTHER),
              (dict(grouping=w.o_grouping, k=0), INVALID, GROUPING_OTHER),
              (dict(grouping=w.unpaired, nq=3), INVALID, "nq=3 exceeds the grouping's max_nq=2"),
              (dict(grouping=w.unpaired), STATE, UNPAIRED),
              (dict(grouping=w.unpaired, qdev=1, null_terms=True), INVALID, "q_terms / q_vals NULL")]   # (the pairing is looked at behind the locks)
    else:
        t += [(dict(k=9), INVALID, "k=9 exceeds the sparse index's max_k=8"),
              (dict(k=9, nq=5), INVALID, "k=9 exceeds the sparse index's max_k=8")]
    return t


def test_refusals_in_order_then_a_good_call(world):
    import torch
    w = world
    for entry in FUSE + SPARSE:
        table = fuse_table(w, entry) if entry in FUSE else sparse_table(w, entry)
        for kw, code, text in table:
            got = call(w, entry, **kw)
            assert got == (code, text), (entry, kw, got)
    for entry in FUSE + SPARSE:   # every lock is free and every staging usable
        assert call(w, entry)[0] == 0, (entry, w.lib.icd_last_error())
        for qdev in ((1,) if entry in SPARSE else ()):
            assert call(w, entry, qdev=qdev)[0] == 0, (entry, "device queries", w.lib.icd_last_error())
    torch.cuda.synchronize()
