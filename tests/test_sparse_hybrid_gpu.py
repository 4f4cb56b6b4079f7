"""icd_fusion_fuse_lists: step 2 of the hybrid search on caller-provided lists. On the lists of a dense
search it equals search_hybrid of the same requests bit for bit; a sparse list next to a dense one fuses by the same rules."""
import os

import numpy as np
import pytest

import sparse_oracle as so
from conftest import GOLDEN
from hybrid_oracle import fuse_query
from rag_project_icd10_amd import _native
from rag_project_icd10_amd.services import sparse_text

pytestmark = pytest.mark.gpu

N, DIM, NQ = 3001, 64, 9


@pytest.fixture(scope="module")
def setup():
    rng = np.random.default_rng(17)
    corpus = rng.standard_normal((N, DIM), dtype=np.float32)
    corpus /= np.linalg.norm(corpus, axis=1, keepdims=True)
    levels = rng.integers(1, 4, N).astype(np.int32)
    index = _native.IcdIndex(corpus, levels, device=0, max_nq=256, max_k=128, probe=False)
    yield index, corpus, levels, rng
    index.close()


@pytest.mark.parametrize("ranker,norm", [("rrf", "none"), ("weighted", "none"), ("weighted", "cosine")])
@pytest.mark.parametrize("R,limits", [(2, [7, 20]), (4, [128, 3, 40, 1])])
def test_fuse_lists_of_a_dense_search_equals_search_hybrid(setup, ranker, norm, R, limits):
    import torch
    index, corpus, levels, _ = setup
    rng = np.random.default_rng(R)
    q = rng.standard_normal((NQ, R, DIM), dtype=np.float32)
    q[:, 1] = q[:, 0] + 0.05 * q[:, 1]   # overlapping lists: ids that several requests hold
    q /= np.linalg.norm(q, axis=2, keepdims=True)
    qd = torch.from_numpy(q).cuda()
    fusion = index.fusion(NQ * R)
    kw = dict(ranker=ranker, weights=[0.7, 0.3, 1.0, 0.0][:R] if ranker == "weighted" else None, norm=norm)
    lmax = max(limits)
    raw, ids = index.search(qd.reshape(NQ * R, DIM), lmax, _native.MODE_EXACT)
    for k in (1, 10, 128):
        for rw in (True, False):
            want = index.search_hybrid(qd, limits, k, fusion, mode=_native.MODE_EXACT, reweighted=rw, **kw)
            got = index.fuse_lists(fusion, raw.reshape(NQ, R, lmax), ids.reshape(NQ, R, lmax), limits, k, reweighted=rw, **kw)
            host = index.fuse_lists(fusion, raw.reshape(NQ, R, lmax).cpu().numpy(), ids.reshape(NQ, R, lmax).cpu().numpy(), limits, k,
                                    reweighted=rw, to_host=True, **kw)
            for w, g, h in zip(want, got, host):
                assert w.cpu().numpy().tobytes() == g.cpu().numpy().tobytes() == h.tobytes()
    fusion.close()


# ---- dense + sparse against tests/hybrid_oracle.py, fed with the two oracles' lists -----------------------------------------------
VOCAB = 37
MIXES = [(2, ("vector", "sparse"), [20, 12]), (4, ("vector", "sparse", "sparse", "vector"), [128, 3, 40, 7])]


@pytest.fixture(scope="module")
def mixed(setup, oracle):
    """device lists and oracle lists of NQ queries for both request mixes: (scores, ids) [NQ, R, lmax] as the device searches
    returned them, and per (query, request) the oracle's unpadded (scores, ids)"""
    index, corpus, levels, _ = setup
    rng = np.random.default_rng(23)
    pairs = [(np.sort(rng.choice(VOCAB, 5, replace=False)).astype(np.uint32), (rng.random(5) * 2 + 0.25).astype(np.float32)) for _ in range(N)]
    rows = sparse_text.csr_from_pairs(pairs)
    sp = index.sparse(*rows, VOCAB, max_nq=64, max_k=128)
    out = {}
    for R, fields, limits in MIXES:
        lmax = max(limits)
        scores = np.full((NQ, R, lmax), -np.inf, np.float32)
        ids = np.full((NQ, R, lmax), -1, np.int64)
        want = [[None] * R for _ in range(NQ)]
        for r, (field, lim) in enumerate(zip(fields, limits)):
            if field == "vector":
                qd = rng.standard_normal((NQ, DIM), dtype=np.float32)
                d_raw, d_ids = index.search(qd, lim, _native.MODE_EXACT)
                o_raw, o_ids = oracle.flat_ip_topk(corpus, qd, lim)
                scores[:, r, :lim], ids[:, r, :lim] = d_raw, d_ids
            else:
                qs = sparse_text.csr_from_pairs([(np.sort(rng.choice(VOCAB, 2, replace=False)).astype(np.uint32), (rng.random(2) + 0.5).astype(np.float32)) for _ in range(NQ)])
                s_raw, s_ids, _ = index.search_sparse(sp, *qs, lim)
                o_raw, o_ids, _ = so.search(*rows, VOCAB, *qs, lim, levels=levels)
                scores[:, r, :lim], ids[:, r, :lim] = s_raw, s_ids
            for q in range(NQ):
                keep = o_ids[q] >= 0
                want[q][r] = (o_raw[q][keep], o_ids[q][keep])
        out[R] = (scores, ids, limits, want)
    yield out
    sp.close()


@pytest.mark.parametrize("R", [2, 4])
@pytest.mark.parametrize("ranker,norm", [("rrf", "none"), ("weighted", "none"), ("weighted", "cosine")])
def test_dense_and_sparse_lists_equal_the_hybrid_oracle(setup, mixed, R, ranker, norm):
    index, corpus, levels, _ = setup
    scores, ids, limits, want = mixed[R]
    for q in range(NQ):   # the device's lists ARE the oracles' lists, bit for bit
        for r in range(R):
            m = len(want[q][r][1])
            assert np.array_equal(ids[q, r, :m], want[q][r][1]) and (ids[q, r, m:limits[r]] == -1).all()
            assert scores[q, r, :m].tobytes() == want[q][r][0].tobytes()
    weights = [0.7, 0.3, 1.0, 0.0][:R]
    fusion = index.fusion(NQ * R)
    for k in (1, 10, 128):
        kw = dict(ranker=ranker, rrf_c=60.0, weights=weights if ranker == "weighted" else None, norm=norm)
        raw = [x.cpu().numpy() for x in index.fuse_lists(fusion, scores, ids, limits, k, reweighted=False, **kw)]
        adj = [x.cpu().numpy() for x in index.fuse_lists(fusion, scores, ids, limits, k, reweighted=True, **kw)]
        for q in range(NQ):
            w_raw, w_adj = fuse_query(want[q], levels, k, ranker, 60.0, weights if ranker == "weighted" else None, norm)
            for g, w in zip(raw, w_raw):
                assert g[q].view(np.uint8).tobytes() == np.asarray(w).astype(g.dtype if w.dtype != np.uint32 else np.int32).view(np.uint8).tobytes(), (k, q)
            for g, w in zip(adj, w_adj):
                assert g[q].view(np.uint8).tobytes() == np.asarray(w).astype(g.dtype if w.dtype != np.uint32 else np.int32).view(np.uint8).tobytes(), (k, q)
    fusion.close()


@pytest.mark.parametrize("R", [2, 4])
def test_dense_and_sparse_lists_under_atan(setup, mixed, R):
    """Weighted with norm atan: the device's atan need not round as the host's does (section 13's rule). Fused scores within
    1e-12; an id is compared only where the oracle's fused score differs from both neighbours' by more than 1e-9 (the first
    hit left out counts as a neighbour). The ranks so left out are at most 5 % - checked here, from the oracle alone."""
    index, corpus, levels, _ = setup
    scores, ids, limits, want = mixed[R]
    weights = [0.7, 0.3, 1.0, 0.5][:R]
    k = 10
    fusion = index.fusion(NQ * R)
    fused, f_ids, _lv, _bits = [x.cpu().numpy() for x in index.fuse_lists(fusion, scores, ids, limits, k, ranker="weighted", weights=weights, norm="atan", reweighted=False)]
    fusion.close()
    total = left_out = 0
    for q in range(NQ):
        (w_f, w_i, _l, _b), _ = fuse_query(want[q], levels, k + 1, "weighted", 60.0, weights, "atan")
        m = int((w_i[:k] >= 0).sum())
        assert int((f_ids[q] >= 0).sum()) == m
        assert np.abs(fused[q, :m] - w_f[:m]).max() <= 1e-12
        for p in range(m):
            total += 1
            near = [w_f[j] for j in (p - 1, p + 1) if 0 <= j <= k and w_i[j] >= 0]
            if any(abs(w_f[p] - x) <= 1e-9 for x in near):
                left_out += 1
                continue
            assert f_ids[q, p] == w_i[p], (q, p)
    assert total > 0 and left_out <= 0.05 * total, (left_out, total)


# ---- services ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def services(tmp_path_factory):
    mp = pytest.MonkeyPatch()
    mp.setenv("MILVUS_DB_PATH", str(tmp_path_factory.mktemp("db")))
    mp.setenv("MILVUS_COLLECTION_NAME", "icd10_sparse")
    mp.setenv("EMBEDDING_MODEL_NAME", "shibing624/text2vec-base-chinese")
    mp.setenv("ICD_EMBEDDING_ALLOW_SYNTHETIC", "1")
    from rag_project_icd10_amd.tools.build_database import DatabaseBuilder
    b = DatabaseBuilder()
    b.initialize_services()
    recs = b.load_csv_data(os.path.join(GOLDEN, "csv_slice.csv"))
    assert b.vectorize_and_index(recs) is True
    yield {"ms": b.milvus_service, "es": b.embedding_service, "recs": recs}
    b.milvus_service.disconnect()
    mp.undo()


def _oracle_hits(recs, texts, k, rows=None):
    titles = [r["preferred_zh"] for r in recs]
    levels = np.array([r.get("level", 1) for r in recs], np.int32)
    vocab, row_off, terms, vals, idf = so.bm25(titles)
    q = sparse_text.csr_from_pairs([so.bm25_query(t, vocab, idf) for t in texts])
    masks = None if rows is None else [rows] * len(texts)
    return so.search(row_off, terms, vals, max(len(vocab), 1), *q, k, levels=levels, masks=masks, reweighted=True)


def test_search_text_on_the_golden_slice(services):
    """Every title of the slice as a query: all hits (codes, BM25 scores, reweighted scores, order) equal the oracle's. The row
    whose title equals the query is rank 0 for every level-1 row: the query's own row holds every query term, and weight 1.2 is
    the largest level weight, so the re-sort cannot put another row in front of a level-1 row that leads by BM25 score. (Rows of
    other levels can be overtaken by a level-1 row through the reweighting, and `伤寒` scores below `伤寒和副伤寒`'s row only
    where both hold the query's terms - the oracle decides those.)"""
    ms, recs = services["ms"], services["recs"]
    titles = [r["preferred_zh"] for r in recs]
    adj, raw, ids, _lv = _oracle_hits(recs, titles, 10)
    level1 = [i for i, r in enumerate(recs) if r.get("level", 1) == 1]
    assert len(level1) >= 10
    for i, t in enumerate(titles):
        hits = ms.search_text(t, 10)
        m = int((ids[i] >= 0).sum())
        assert [h["code"] for h in hits] == [recs[j]["code"] for j in ids[i][:m]], t
        assert [h["original_score"] for h in hits] == [float(x) for x in raw[i][:m]] and [h["score"] for h in hits] == [float(x) for x in adj[i][:m]]
        if i in level1:
            assert hits[0]["title"] == t
    assert ms.search_text("zzzzqqq", 5) == [] and ms.search_text("", 5) == []   # no term of the vocabulary: no hit
    # a filter goes through the mask cache; the batch form returns arrays
    sel = np.array([r.get("level", 1) >= 3 for r in recs])
    f_adj, f_raw, f_ids, _ = _oracle_hits(recs, titles[:5], 7, rows=sel)
    tx = ms.build_sparse_index()[1]
    g_adj, g_raw, g_ids, g_lv = ms.search_sparse_batch(*tx.encode_queries(titles[:5]), 7, filter="level >= 3")
    assert np.array_equal(g_ids, f_ids) and g_raw.tobytes() == f_raw.tobytes() and g_adj.tobytes() == f_adj.tobytes()
    assert [h["code"] for h in ms.search_text(titles[0], 7, filter="level >= 3")] == [recs[j]["code"] for j in f_ids[0] if j >= 0]
    st = ms.sparse_indexes()
    assert len(st) == 1 and st[0]["field"] == "preferred_zh" and st[0]["vocab"] == tx.vocab_size and st[0]["nnz"] == len(tx.terms) and st[0]["bytes"] > 0
    with pytest.raises(ValueError):
        ms.search_text(titles[0], 0)
    with pytest.raises(ValueError):
        ms.search_text(titles[0], 5, filter="level >>> 3")


def test_service_hybrid_search_with_a_sparse_request_and_the_endpoint(services):
    # (last of the module: the app's lifespan disconnects the installed services when the client closes)
    from fastapi.testclient import TestClient
    from rag_project_icd10_amd.api import app as appmod
    from rag_project_icd10_amd.services.hybrid_search import AnnSearchRequest, RRFRanker, WeightedRanker
    ms, es, recs = services["ms"], services["es"], services["recs"]
    levels = ms.client.levels()
    texts = [recs[40]["preferred_zh"], recs[41]["preferred_zh"] + " I10"]
    vecs = np.asarray(es.encode_query_batch(texts), dtype=np.float32)

    def lists_for(i, limits, expr=None):
        kw = {} if expr is None else {"filter": expr, "filter_mode": "mask"}
        _a, d_raw, d_ids, _l = ms.search_batch(vecs[i][None, :], limits[0], **kw)
        keep = d_ids[0] >= 0
        order = np.lexsort((d_ids[0][keep], -d_raw[0][keep].astype(np.float64)))
        sel = None if expr is None else np.array([r.get("level", 1) >= 2 for r in recs])
        _sa, s_raw, s_ids, _sl = _oracle_hits(recs, [texts[i]], limits[1], rows=sel)
        s_keep = s_ids[0] >= 0
        s_order = np.lexsort((s_ids[0][s_keep], -s_raw[0][s_keep].astype(np.float64)))
        return [(d_raw[0][keep][order], d_ids[0][keep][order]), (s_raw[0][s_keep][s_order], s_ids[0][s_keep][s_order])]

    for ranker, okw in ((RRFRanker(60), dict(ranker="rrf", c=60.0)), (WeightedRanker(0.6, 0.4, norm_score="none"), dict(ranker="weighted", weights=[0.6, 0.4], norm="none"))):
        for expr in (None, "level >= 2"):
            for i in range(2):
                limits = [20, 9]
                reqs = [AnnSearchRequest(vecs[i], limits[0], expr=expr), AnnSearchRequest(texts[i], limits[1], expr=expr, anns_field="sparse")]
                _raw, (adj, fused, ids, _lv, bits) = fuse_query(lists_for(i, limits, expr), levels, 10, **okw)
                hits = ms.hybrid_search(reqs, ranker, 10)
                m = int((ids >= 0).sum())
                assert [h["code"] for h in hits] == [recs[j]["code"] for j in ids[:m]], (okw, expr, i)
                assert [h["score"] for h in hits] == [float(a) for a in adj[:m]] and [h["fused_score"] for h in hits] == [float(f) for f in fused[:m]]
                assert [h["matched_requests"] for h in hits] == [[r for r in range(2) if (int(b) >> r) & 1] for b in bits[:m]]
    # a {term_id: weight} dict is a sparse request too; a batch of texts; a sparse request alone
    tx = ms.build_sparse_index()[1]
    t, w = tx.encode_query(texts[0])
    as_dict = ms.hybrid_search([AnnSearchRequest(vecs[0], 20), AnnSearchRequest({int(a): float(b) for a, b in zip(t, w)}, 9, anns_field="sparse")], RRFRanker(60), 10)
    as_text = ms.hybrid_search([AnnSearchRequest(vecs[0], 20), AnnSearchRequest(texts[0], 9, anns_field="sparse")], RRFRanker(60), 10)
    assert as_dict == as_text
    batch = ms.hybrid_search_batch([AnnSearchRequest(vecs, 20), AnnSearchRequest(texts, 9, anns_field="sparse")], RRFRanker(60), 10, as_dicts=True)
    assert batch[0] == as_text and len(batch) == 2
    alone = ms.hybrid_search([AnnSearchRequest(texts[0], 9, anns_field="sparse")], WeightedRanker(1.0, norm_score="none"), 9)
    assert [h["code"] for h in alone] == [h["code"] for h in ms.search_text(texts[0], 9)]
    with pytest.raises(ValueError):
        ms.hybrid_search_batch([AnnSearchRequest(vecs, 20), AnnSearchRequest(texts[:1], 9, anns_field="sparse")], RRFRanker(60), 10)
    appmod.install_services(es, ms)
    try:
        with TestClient(appmod.app) as client:
            plain = client.post("/query", json={"text": texts[0], "top_k": 5})
            r = client.post("/hybrid_query", json={"texts": texts, "top_k": 5, "req_limit": 20, "sparse": True})
            assert r.status_code == 200, r.text
            body = r.json()
            if plain.status_code == 200:
                assert set(body.keys()) == set(plain.json().keys())
                if plain.json()["candidates"]:
                    assert set(body["candidates"][0].keys()) == set(plain.json()["candidates"][0].keys())
            reqs = [AnnSearchRequest(vecs[i], 20) for i in range(2)] + [AnnSearchRequest(t_, 20, anns_field="sparse") for t_ in texts]
            want = ms.hybrid_search(reqs, RRFRanker(60), 5)
            assert [c["code"] for c in body["candidates"]] == [h["code"] for h in want]
            assert [c["original_score"] for c in body["candidates"]] == [h["fused_score"] for h in want]
            assert any(2 in c["similarity_factors"]["matched_requests"] or 3 in c["similarity_factors"]["matched_requests"] for c in body["candidates"])
            assert client.post("/hybrid_query", json={"texts": texts * 3, "sparse": True}).status_code == 400   # 12 requests
            assert client.post("/hybrid_query", json={"texts": texts, "sparse": True, "ranker": {"strategy": "weighted", "params": {"weights": [0.5, 0.5]}}}).status_code == 400
            stats = client.get("/stats").json()
            assert stats["sparse_indexes"][0]["field"] == "preferred_zh" and stats["sparse_indexes"][0]["nnz"] > 0
    finally:
        appmod.install_services(None, None, None)
