"""Grouped hybrid search on the device (rules H1 - H6) against tests/grouped_hybrid_oracle.py: ids, levels,
request bits, groups, fused and adjusted doubles bit for bit under RRF and Weighted none / cosine; atan within 1e-12. The corpus is
the family-shaped one of tests/test_grouped_search_gpu.py (120 rows around a centre, dim 768) at n = 3 000; the full ranking of one
pool of vectors is computed once and shared."""
import ctypes

import numpy as np
import pytest

import grouped_hybrid_oracle as gho
import sparse_oracle as so
from conftest import icd_levels
from rag_project_icd10_amd import _native
from rag_project_icd10_amd._native import MODE_EXACT, IcdIndex

pytestmark = pytest.mark.gpu

N, DIM, POOL = 3000, 768, 320
ROWS = np.arange(N, dtype=np.int64)
# families of 120; `mixed`: every 50th row leaves its family for a group of TWO rows (a run shorter than s = 3); `seven`: fewer
# groups than k = 10; `own`: every row its own group
GROUPINGS = {"family": ROWS // 120, "mixed": np.where(ROWS % 50 == 0, 1000 + ROWS // 100, ROWS // 120), "seven": ROWS % 7,
             "own": (ROWS * 7 + 1) % N}
WEIGHTS = [0.3, 1.0, 0.7, 0.9, 0.2, 0.6, 0.1, 0.8]
_S = {}


def setup(oracle):
    if not _S:
        rng = np.random.default_rng(3)
        cent = rng.standard_normal((N // 120, DIM)).astype(np.float32)
        x = np.repeat(cent, 120, axis=0) + 0.35 * rng.standard_normal((N, DIM)).astype(np.float32)
        x = np.ascontiguousarray(x / np.linalg.norm(x, axis=1, keepdims=True), dtype=np.float32)
        pool = np.ascontiguousarray(x[rng.integers(0, N, POOL)] + 0.05 * rng.standard_normal((POOL, DIM)).astype(np.float32), dtype=np.float32)
        levels = icd_levels(N, 7)
        s_all, i_all = oracle.flat_ip_topk(x, pool, N)
        index = IcdIndex(x, levels, max_nq=2400, max_k=128)
        _S.update(corpus=x, pool=pool, levels=levels, s=s_all, i=i_all, index=index, fusion=index.fusion(2400), groupings={})
    return _S


def grouping(st, name):
    if name not in st["groupings"]:
        st["groupings"][name] = st["index"].grouping(GROUPINGS[name].astype(np.int32), max_nq=2400)
    return st["groupings"][name]


def sel_for(nq, R, seed):
    """request r of query q: a pool vector; neighbouring requests of a query are near one another, so that the lists overlap"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, POOL, nq)
    return (base[:, None] + rng.integers(0, 3, (nq, R))) % POOL


def same(got, want, what):
    names = ("adj", "fused", "ids", "levels", "bits", "groups")[6 - len(want):]
    assert len(got) == len(want), what
    for g, w, name in zip(got, want, names):
        g = g.cpu().numpy() if hasattr(g, "cpu") else g
        if name == "bits":
            g, w = g.view(np.uint32), w.view(np.uint32)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        bad = np.flatnonzero((g.view(np.uint8).reshape(g.shape[0], -1) != w.view(np.uint8).reshape(w.shape[0], -1)).any(axis=1))
        assert bad.size == 0, f"{what}: {name} differs in queries {bad[:8].tolist()}: {g[bad[0]][:6]} vs {w[bad[0]][:6]}"


# (R, limits in groups, (k, s), nq, grouping, ranker, norm)
CASES = [(1, [7], (1, 1), 1, "family", "rrf", "none"),
         (2, [10, 4], (10, 1), 4, "family", "weighted", "none"),
         (3, [5, 9, 2], (5, 3), 17, "mixed", "weighted", "cosine"),
         (8, [4, 3, 2, 4, 1, 4, 2, 3], (4, 32), 300, "family", "rrf", "none"),
         (2, [128, 60], (10, 1), 17, "mixed", "weighted", "none"),
         (3, [4, 4, 2], (4, 32), 4, "mixed", "rrf", "none"),
         (2, [9, 5], (10, 1), 17, "seven", "rrf", "none"),
         (3, [6, 3, 8], (5, 3), 17, "own", "weighted", "cosine")]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_grouped_hybrid_search_equals_the_oracle(oracle, case):
    import torch
    R, limits, (k, s), nq, gname, ranker, norm = CASES[case]
    st = setup(oracle)
    index, fusion, g = st["index"], st["fusion"], grouping(st, gname)
    sel = sel_for(nq, R, case)
    kw = dict(ranker=ranker, weights=WEIGHTS[:R] if ranker == "weighted" else None, norm=norm)
    want_raw, want_adj, _ = gho.hybrid_grouped_batch(st["s"], st["i"], GROUPINGS[gname], st["levels"], sel, limits, k, s, ranker, 60.0, kw["weights"], norm)
    q = np.ascontiguousarray(st["pool"][sel])
    same(index.search_hybrid(q, limits, k, fusion, reweighted=False, grouping=g, group_size=s, **kw), want_raw, f"host raw {CASES[case]}")
    same(index.search_hybrid(q, limits, k, fusion, reweighted=True, grouping=g, group_size=s, **kw), want_adj, f"host reweighted {CASES[case]}")
    got = index.search_hybrid(torch.from_numpy(q).cuda(), limits, k, fusion, reweighted=True, grouping=g, group_size=s, **kw)
    assert all(t.is_cuda for t in got)
    same(got, want_adj, f"device {CASES[case]}")
    hits = (want_raw[1] >= 0).sum(axis=1)
    if gname == "seven":   # fewer fused groups than k: padding behind them
        assert (hits < k * s).all() and (want_raw[4][:, -1] == -1).all() and np.isneginf(want_raw[0][:, -1]).all()
    if gname == "mixed" and s == 3:   # a run shorter than s in front of a cut: slots, not runs, would cut elsewhere
        sub = gho.go.Ranking(st["s"][sel[:, 0]], st["i"][sel[:, 0]], GROUPINGS[gname]).raw(limits[0], s)[1]
        assert (((sub >= 0).sum(axis=1)) < limits[0] * s).any()


def test_weighted_atan_within_1e_12_of_the_oracle(oracle):
    """the device's atan need not round as the host's does: fused and adjusted scores within 1e-12. Ids, levels, bits and groups are
    compared for every query whose fused heads are pairwise more than 1e-9 apart (then no comparison of rule H3 can go the other
    way); the others are left out, capped at 10 % of the ranks. On these inputs the oracle leaves out 0.0 % (measured on the CPU:
    distinct weights and noisy copies keep the heads apart)."""
    st = setup(oracle)
    index, fusion = st["index"], st["fusion"]
    compared = total = 0
    for R, limits, (k, s), nq, gname in ((3, [10, 6, 4], (5, 3), 17, "mixed"), (8, [4] * 8, (4, 32), 17, "family"), (2, [10, 10], (10, 1), 300, "family")):
        sel = sel_for(nq, R, 100 + R)
        _, want, gaps = gho.hybrid_grouped_batch(st["s"], st["i"], GROUPINGS[gname], st["levels"], sel, limits, k, s, "weighted", 60.0, WEIGHTS[:R], "atan")
        got = index.search_hybrid(np.ascontiguousarray(st["pool"][sel]), limits, k, fusion, ranker="weighted", weights=WEIGHTS[:R], norm="atan",
                                  grouping=grouping(st, gname), group_size=s)
        clear = gaps > 1e-9
        valid = want[2] >= 0
        total += int(valid.sum())
        compared += int(valid[clear].sum())
        for j in (2, 3, 4, 5):
            assert np.array_equal(np.asarray(got[j])[clear].astype(np.int64), want[j][clear].astype(np.int64)), (R, j)
        for j in (0, 1):
            err = np.abs(got[j][clear][valid[clear]] - want[j][clear][valid[clear]]).max()
            print(f"atan R={R}: max |{('adj', 'fused')[j]} - oracle| = {err:.3e}")
            assert err <= 1e-12
    print(f"atan: {compared} of {total} ranks compared by id")
    assert compared >= 0.9 * total


def test_h5_identities_against_the_index_itself(oracle):
    st = setup(oracle)
    index, fusion = st["index"], st["fusion"]
    own, fam = grouping(st, "own"), grouping(st, "family")
    sel = sel_for(17, 3, 9)
    q = np.ascontiguousarray(st["pool"][sel])
    for ranker, norm in (("rrf", "none"), ("weighted", "cosine")):
        kw = dict(ranker=ranker, weights=WEIGHTS[:3] if ranker == "weighted" else None, norm=norm)
        for rw in (False, True):
            plain = index.search_hybrid(q, [10, 40, 7], 10, fusion, mode=MODE_EXACT, reweighted=rw, **kw)
            got = index.search_hybrid(q, [10, 40, 7], 10, fusion, reweighted=rw, grouping=own, group_size=1, **kw)
            same(got[:-1], plain, f"own groups, s = 1, {ranker} rw={rw}")
    q1 = np.ascontiguousarray(st["pool"][:40])
    for k, s in ((10, 1), (5, 3), (4, 32)):
        raw, ids, lv, grp = index.search_grouped(q1, k, s, fam, reweighted=False)
        fused, hid, hlv, bits, hgrp = index.search_hybrid(q1[:, None, :], [k], k, fusion, ranker="weighted", weights=[1.0], norm="none",
                                                          reweighted=False, grouping=fam, group_size=s)
        assert np.array_equal(hid, ids) and np.array_equal(hlv, lv) and np.array_equal(hgrp, grp) and fused.tobytes() == raw.astype(np.float64).tobytes()
        assert (bits[hid >= 0] == 1).all()


def test_a_view_uses_its_own_grouping(oracle):
    st = setup(oracle)
    rows = np.flatnonzero(ROWS % 3 != 1)
    view = st["index"].view(rows, max_nq=64, max_k=128)
    g_of = GROUPINGS["mixed"][rows]
    vg, vf = view.grouping(g_of.astype(np.int32), max_nq=64), view.fusion(64)
    pool = st["pool"][:32]
    s_v, i_v = oracle.flat_ip_topk(np.ascontiguousarray(st["corpus"][rows]), pool, len(rows))
    sel = sel_for(9, 3, 4) % 32
    want_raw, want_adj, _ = gho.hybrid_grouped_batch(s_v, i_v, g_of, st["levels"], sel, [6, 3, 8], 5, 3, "rrf", row_map=rows)
    q = np.ascontiguousarray(pool[sel])
    same(view.search_hybrid(q, [6, 3, 8], 5, vf, reweighted=False, grouping=vg, group_size=3), want_raw, "view raw")
    same(view.search_hybrid(q, [6, 3, 8], 5, vf, grouping=vg, group_size=3), want_adj, "view reweighted")
    with pytest.raises(ValueError):
        view.search_hybrid(q, [6, 3, 8], 5, vf, grouping=grouping(st, "mixed"), group_size=3)   # the parent's grouping is another index's
    for x in (vg, vf, view):
        x.close()


@pytest.mark.parametrize("R", [2, 4])
def test_dense_and_sparse_lists_fused_with_grouping(oracle, R):
    """caller-provided lists: dense grouped lists next to PLAIN sparse lists (runs of any length, in the list's own order), cut by
    runs and fused with grouping, against the oracle"""
    st = setup(oracle)
    index, fusion, g = st["index"], st["fusion"], grouping(st, "mixed")
    group_of, nq, s, k, lmax = GROUPINGS["mixed"], 17, 3, 5, 30
    rng = np.random.default_rng(R)
    terms = np.sort(rng.integers(0, 50, (N, 4)), axis=1)
    pairs = [(np.unique(t).astype(np.uint32), (np.arange(len(np.unique(t))) + 1).astype(np.float32) / 2) for t in terms]
    row_off = np.cumsum([0] + [len(p[0]) for p in pairs]).astype(np.int64)
    sp_rows = (row_off, np.concatenate([p[0] for p in pairs]), np.concatenate([p[1] for p in pairs]))
    sp = index.sparse(*sp_rows, 50, max_nq=64, max_k=128)
    qp = [(np.unique(rng.integers(0, 50, 3)).astype(np.uint32), np.ones(1, np.float32)) for _ in range(nq)]
    qp = [(t, np.full(len(t), 1.5, np.float32)) for t, _ in qp]
    q_off = np.cumsum([0] + [len(t) for t, _ in qp]).astype(np.int64)
    sq = (q_off, np.concatenate([t for t, _ in qp]), np.concatenate([v for _, v in qp]))
    sp_raw, sp_ids, _ = so.search(*sp_rows, 50, *sq, lmax)
    got_sp = index.search_sparse(sp, *sq, lmax)
    assert np.array_equal(got_sp[1], sp_ids)
    sel = sel_for(nq, R, 20 + R)
    d_raw, d_ids, _ = gho.go.Ranking(st["s"], st["i"], group_of).raw(lmax // s, s)
    limits = [4, 6, 3, 10][:R]
    lists_s = np.stack([np.stack([sp_raw if r % 2 else d_raw[sel[:, r]] for r in range(R)], axis=1)])[0]
    lists_i = np.stack([np.stack([sp_ids if r % 2 else d_ids[sel[:, r]] for r in range(R)], axis=1)])[0]
    for ranker, norm in (("rrf", "none"), ("weighted", "cosine")):
        w = WEIGHTS[:R] if ranker == "weighted" else None
        outs = [gho.fuse_query_grouped([(lists_s[q, r], lists_i[q, r]) for r in range(R)], group_of, st["levels"], limits, k, s, ranker, 60.0, w, norm)
                for q in range(nq)]
        want_raw = tuple(np.stack([o[0][j] for o in outs]) for j in range(5))
        want_adj = tuple(np.stack([o[1][j] for o in outs]) for j in range(6))
        same(index.fuse_lists(fusion, lists_s, lists_i, limits, k, ranker=ranker, weights=w, norm=norm, reweighted=False, to_host=True,
                              grouping=g, group_size=s), want_raw, f"lists raw R={R} {ranker}")
        same(index.fuse_lists(fusion, lists_s, lists_i, limits, k, ranker=ranker, weights=w, norm=norm, grouping=g, group_size=s), want_adj,
             f"lists reweighted R={R} {ranker}")
    sp.close()


def test_refusals(oracle):
    st = setup(oracle)
    lib = _native.load_library()
    index, fusion, g = st["index"], st["fusion"], grouping(st, "family")
    q = np.ascontiguousarray(st["pool"][:4].reshape(2, 2, DIM))
    lim = np.array([3, 3], np.int32)
    out = [np.empty((2, 128), dt) for dt in (np.float64, np.float64, np.int64, np.int32, np.uint32, np.int32)]

    def call(idx_h, f_h, g_h, R=2, limits=lim, masks=None, radius=None, rf=None, k=3, s=2, nq=2):
        return lib.icd_index_search_hybrid_grouped(idx_h, f_h, g_h, q.ctypes.data, nq, R, 0, limits.ctypes.data, masks, radius, rf, 0, 60.0, None, 0,
                                                   k, s, 1, *[o.ctypes.data for o in out], 0, None)
    assert call(index._h, fusion._h, g._h) == 0
    for k, s in ((0, 1), (1, 0), (129, 1), (10, 13)):
        assert call(index._h, fusion._h, g._h, k=k, s=s) == -1 and b"k * group_size" in lib.icd_last_error()
    assert call(index._h, fusion._h, g._h, limits=np.array([3, 33], np.int32), k=1, s=4) == -1 and b"limits[1]" in lib.icd_last_error()
    assert call(index._h, fusion._h, g._h, limits=np.array([0, 3], np.int32)) == -1
    mask = index.rowmask(np.arange(10))
    table = (ctypes.c_void_p * 4)(mask._h.value, None, None, None)
    assert call(index._h, fusion._h, g._h, masks=table) == -1 and b"grouping" in lib.icd_last_error()
    band = np.zeros(4, np.float32)
    assert call(index._h, fusion._h, g._h, radius=band.ctypes.data) == -1 and call(index._h, fusion._h, g._h, rf=band.ctypes.data) == -1
    other = IcdIndex(st["corpus"][:500], st["levels"][:500], max_nq=8, max_k=16)
    og, of = other.grouping((np.arange(500) % 5).astype(np.int32)), other.fusion(8)
    assert call(index._h, fusion._h, og._h) == -1 and b"another index" in lib.icd_last_error()
    assert call(index._h, of._h, g._h) == -1 and b"another index" in lib.icd_last_error()
    small_g, small_f = index.grouping(GROUPINGS["family"].astype(np.int32), max_nq=3), index.fusion(3)
    assert call(index._h, fusion._h, small_g._h) == -1 and b"grouping's max_nq" in lib.icd_last_error()
    assert call(index._h, small_f._h, g._h) == -1 and b"max_total" in lib.icd_last_error()
    sc, ids = np.zeros(1, np.float32), np.zeros(1, np.int64)
    assert lib.icd_fusion_fuse_lists_grouped(index._h, fusion._h, og._h, sc.ctypes.data, ids.ctypes.data, 2, 2, 8, lim.ctypes.data, 0, 60.0, None, 0, 3, 2, 1,
                                             *[o.ctypes.data for o in out], 0, None) == -1
    assert lib.icd_fusion_fuse_lists_grouped(index._h, fusion._h, g._h, sc.ctypes.data, ids.ctypes.data, 2, 2, 8, lim.ctypes.data, 0, 60.0, None, 0, 10, 13, 1,
                                             *[o.ctypes.data for o in out], 0, None) == -1
    dead = ctypes.c_void_p(small_g._h.value)
    small_g.close()
    assert call(index._h, fusion._h, dead) == -5   # ICD_ERR_STATE
    with pytest.raises(ValueError):
        index.search_hybrid(q, [3, 3], 3, fusion, grouping=g, group_size=2, masks=[[mask, None], [None, None]])
    with pytest.raises(ValueError):
        index.search_hybrid(q, [3, 3], 3, fusion, grouping=g, group_size=2, radius=0.1)
    with pytest.raises(ValueError):
        index.search_hybrid(q, [3, 3], 3, fusion, group_size=2)
    # any destruction order: a grouping and a fusion outlive their index
    other.close()
    assert og.stats()["groups"] == 5
    for x in (og, of, small_f, mask):
        x.close()


# ---- the service and the endpoint ---------------------------------------------------------------------------------------------------
from test_sparse_hybrid_gpu import services   # noqa: E402,F401  (the golden slice behind MilvusService, built once for this module)


def test_service_hybrid_search_grouped_and_the_endpoint(services, oracle):   # noqa: F811
    """MilvusService.hybrid_search(..., group_by_field=) on the golden slice against the oracle: dense requests (on the expression's
    view with the view's grouping) and dense + sparse (the sparse side on the parent under the mask, fused on the parent), then
    /hybrid_query with grouping. main_code is unique per row of the slice (the identity grouping); parent_code makes 81 families.
    (last of the module: the app's lifespan disconnects the installed services when the client closes)"""
    from fastapi.testclient import TestClient
    from rag_project_icd10_amd.api import app as appmod
    from rag_project_icd10_amd.services import sparse_text
    from rag_project_icd10_amd.services.hybrid_search import AnnSearchRequest, RRFRanker, WeightedRanker
    ms, es, recs = services["ms"], services["es"], services["recs"]
    corpus, levels = ms.client.matrix(), ms.client.levels()
    n = len(recs)
    texts = [recs[40]["preferred_zh"], recs[41]["preferred_zh"] + " I10"]
    vecs = np.asarray(es.encode_query_batch(texts), dtype=np.float32)
    titles = [r["preferred_zh"] for r in recs]
    vocab, row_off, terms, vals, idf = so.bm25(titles)
    sq = sparse_text.csr_from_pairs([so.bm25_query(t, vocab, idf) for t in texts])
    rankers = ((RRFRanker(60), dict(ranker="rrf", c=60.0)), (WeightedRanker(0.6, 0.4, norm_score="none"), dict(ranker="weighted", weights=[0.6, 0.4], norm="none")))

    def check(hits, adj, fused, ids, bits, grp, values, field, what):
        m = int((ids >= 0).sum())
        assert [h["code"] for h in hits] == [recs[j]["code"] for j in ids[:m]], what
        assert [h["score"] for h in hits] == [float(a) for a in adj[:m]] and [h["fused_score"] for h in hits] == [float(f) for f in fused[:m]], what
        assert [h["matched_requests"] for h in hits] == [[r for r in range(2) if (int(b) >> r) & 1] for b in bits[:m]], what
        assert [h["metadata"][field] for h in hits] == [values[g] for g in grp[:m]], what

    for field, (k, s) in (("main_code", (5, 1)), ("parent_code", (5, 3))):
        values, group_all = np.unique(np.array([str(r.get(field) or "") for r in recs]), return_inverse=True)
        for expr in (None, "level >= 2"):
            rows = np.arange(n, dtype=np.int64) if expr is None else ms.filter_rows(expr)
            sel = np.zeros(n, bool)
            sel[rows] = True
            s_all, i_all = oracle.flat_ip_topk(np.ascontiguousarray(corpus[rows]), vecs, len(rows))
            for ranker, okw in rankers:
                # two dense requests
                _raw, want, _gap = gho.hybrid_grouped_batch(s_all, i_all, group_all[rows], levels, [[0, 1]], [6, 4], k, s, row_map=rows, **okw)
                hits = ms.hybrid_search([AnnSearchRequest(vecs[0], 6, expr=expr), AnnSearchRequest(vecs[1], 4, expr=expr)], ranker, k,
                                        group_by_field=field, group_size=s)
                check(hits, want[0][0], want[1][0], want[2][0], want[4][0], want[5][0], values, field, (field, expr, okw, "dense"))
                assert len({h["metadata"][field] for h in hits}) <= k
                # a dense and a sparse request of the same text
                d_s, d_i, _ = gho.go.Ranking(s_all[:1], i_all[:1], group_all[rows]).raw(6, s)
                r_raw, r_ids = gho.sparse_ranking(row_off, terms, vals, max(len(vocab), 1), sq[0][:2], sq[1][:sq[0][1]], sq[2][:sq[0][1]],
                                                  masks=None if expr is None else [sel])
                p_s, p_i, _ = gho.Ranking(r_raw, r_ids, group_all).raw(4, s)
                lists = [(d_s[0], np.where(d_i[0] >= 0, rows[np.clip(d_i[0], 0, None)], -1)), (p_s[0], p_i[0])]
                _r, w2, _g = gho.fuse_query_grouped(lists, group_all, levels, [6, 4], k, s, **okw)
                hits = ms.hybrid_search([AnnSearchRequest(vecs[0], 6, expr=expr), AnnSearchRequest(texts[0], 4, expr=expr, anns_field="sparse")], ranker, k,
                                        group_by_field=field, group_size=s)
                check(hits, w2[0], w2[1], w2[2], w2[4], w2[5], values, field, (field, expr, okw, "dense + sparse"))
    arrays = ms.hybrid_search_batch([AnnSearchRequest(vecs, 6), AnnSearchRequest(vecs[::-1].copy(), 4)], RRFRanker(60), 5, group_by_field="parent_code", group_size=3)
    assert len(arrays) == 6 and arrays[2].shape == (2, 15)
    assert ms.hybrid_search([AnnSearchRequest(vecs[0], 6, expr='code like "ZZZ%"')], RRFRanker(60), 5, group_by_field="parent_code") == []   # no row selected
    v = vecs[0]
    for bad_reqs, kw in (([AnnSearchRequest(v, 6, expr="level >= 2"), AnnSearchRequest(v, 6)], dict(group_by_field="parent_code")),
                         ([AnnSearchRequest(v, 6, expr="level >= 2"), AnnSearchRequest(v, 6, expr="level >= 3")], dict(group_by_field="parent_code")),
                         ([AnnSearchRequest(v, 6, param={"radius": 0.1})], dict(group_by_field="parent_code")),
                         ([AnnSearchRequest(v, 50)], dict(group_by_field="parent_code", group_size=3)),
                         ([AnnSearchRequest(v, 6)], dict(group_size=3))):
        with pytest.raises(ValueError):
            ms.hybrid_search(bad_reqs, RRFRanker(60), 5, **kw)
    appmod.install_services(es, ms)
    try:
        with TestClient(appmod.app) as client:
            body = {"texts": texts, "top_k": 5, "req_limit": 6, "group_by_field": "parent_code", "group_size": 3}
            r = client.post("/hybrid_query", json=body)
            assert r.status_code == 200, r.text
            want = ms.hybrid_search([AnnSearchRequest(vecs[i], 6) for i in range(2)], RRFRanker(60), 5, group_by_field="parent_code", group_size=3)
            got = r.json()["candidates"]
            assert [c["code"] for c in got] == [h["code"] for h in want] and [c["original_score"] for c in got] == [h["fused_score"] for h in want]
            assert len(got) > 5 and len({c["parent_code"] for c in got}) <= 5
            r = client.post("/hybrid_query", json={**body, "sparse": True, "filter": "level >= 2"})
            assert r.status_code == 200 and r.json()["candidates"], r.text
            for patch in ({"group_by_field": "nope"}, {"group_size": 0}, {"group_size": 26}, {"req_limit": 50}, {"group_by_field": None}):
                assert client.post("/hybrid_query", json={**body, **patch}).status_code == 400, patch
    finally:
        appmod.install_services(None, None, None)
