"""MilvusService.search_by_ids / similar_codes / knn_graph on the golden CSV slice's store, with the test
encoder weights the neighbouring service tests use: the batch forms against one search_by_ids call per row, against search_batch of
the HOST copies of the stored vectors at k + 1 with the row's own hit dropped in numpy, and against tests/byrows_oracle.py; per-id
filters (a TEXT_MATCH one among them) with the masks made on the device and on the host; the API route. Exact: no tolerance."""
import os

import numpy as np
import pytest

import byrows_oracle as bo

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILTERS = ['level >= 2 and code like "A0%"', 'not (level == 1 or (code like "A01%" and not has_complication == true))',
           'parent_code != "" and (level in [2] or secondary_code like "G%")', 'level >= 2 and TEXT_MATCH(preferred_zh, "伤寒")']
K = 10


@pytest.fixture(scope="module")
def services(tmp_path_factory):
    mp = pytest.MonkeyPatch()
    mp.setenv("MILVUS_DB_PATH", str(tmp_path_factory.mktemp("db")))
    mp.setenv("MILVUS_COLLECTION_NAME", "icd10_byrows")
    mp.setenv("EMBEDDING_MODEL_NAME", "shibing624/text2vec-base-chinese")
    mp.setenv("ICD_EMBEDDING_ALLOW_SYNTHETIC", "1")
    from rag_project_icd10_amd.tools.build_database import DatabaseBuilder
    b = DatabaseBuilder()
    b.initialize_services()
    recs = b.load_csv_data(os.path.join(GOLDEN, "csv_slice.csv"))[:300]
    assert b.vectorize_and_index(recs) is True
    yield {"ms": b.milvus_service, "es": b.embedding_service}
    b.milvus_service.disconnect()
    mp.undo()


@pytest.fixture(scope="module")
def world(services, oracle):
    """the stored vectors, the oracle's full ranking of each against the store, the filters' selections: computed once"""
    ms = services["ms"]
    corpus = np.ascontiguousarray(ms.client.matrix(), np.float32)
    levels = np.asarray(ms.client.levels(), np.int32)
    n = len(corpus)
    assert 100 <= n <= 300
    fs, fi = oracle.flat_ip_topk(corpus, corpus, n)
    keep = {e: None if e is None else np.isin(np.arange(n), ms.filter_rows(e)) for e in FILTERS + [None]}
    assert all(0 < keep[e].sum() < n for e in FILTERS)
    return {"corpus": corpus, "levels": levels, "n": n, "fs": fs, "fi": fi, "keep": keep}


def arrays(out):
    return [np.asarray(x.cpu().numpy() if hasattr(x, "cpu") else x) for x in out]


def same(got, want, what):
    for j, (g, w) in enumerate(zip(arrays(got), arrays(want))):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (what, j, g, w)


def want(world, ids, k, filters, **kw):
    ids = np.asarray(ids, np.int64)
    return bo.byrows_batch(world["fs"][ids], world["fi"][ids], world["levels"], ids, k, masks=[world["keep"][e] for e in filters], **kw)[1]


def check_routes(ms, world):
    n = world["n"]
    every = np.arange(n, dtype=np.int64)
    # the whole slice in one call: one call per row, the oracle, and the host route a caller has without the entry point
    batch = ms.search_by_ids(every, K)
    same(batch, want(world, every, K, [None] * n), "the oracle")
    for r in (0, 1, n // 2, n - 1):
        same(ms.search_by_ids([r], K), [x[r:r + 1] for x in batch], ("one call per row", r))
    for r in range(0, n, 7):
        same(ms.search_by_ids(int(r), K), [x[r:r + 1] for x in batch], ("one call per row", r))
    wide = arrays(ms.search_batch(world["corpus"], K + 1, filter=[None] * n))       # host vectors, the mask path: exact, at k + 1
    cut = [bo.drop_reweighted_list(wide[0][q], wide[1][q], wide[2][q], wide[3][q], q) for q in range(n)]
    same(batch, [np.stack([c[j] for c in cut]) for j in range(4)], "search_batch at k + 1, self dropped")
    same(ms.search_by_ids(every, K, include_self=True), ms.search_batch(world["corpus"], K, filter=[None] * n), "include_self is search_batch")
    # knn_graph: every row's list, ids and adjusted scores; the raw form; under one filter
    g_ids, g_scores = ms.knn_graph(K)
    assert g_ids.dtype == np.int64 and g_scores.dtype == np.float64 and g_ids.shape == g_scores.shape == (n, K)
    assert g_ids.tobytes() == arrays(batch)[2].tobytes() and g_scores.tobytes() == arrays(batch)[0].tobytes()
    assert (g_ids != every[:, None]).all()
    r_ids, r_scores = ms.knn_graph(K, reweighted=False)
    raw = bo.byrows_batch(world["fs"], world["fi"], world["levels"], every, K)[0]
    assert r_ids.tobytes() == raw[1].tobytes() and r_scores.tobytes() == raw[0].astype(np.float64).tobytes()
    for e in (FILTERS[0], FILTERS[3]):
        f_ids, f_scores = ms.knn_graph(K, filter=e)
        w = want(world, every, K, [e] * n)
        assert f_ids.tobytes() == w[2].tobytes() and f_scores.tobytes() == w[0].tobytes(), e
        same(ms.search_by_ids(every, K, filter=e), w, e)
    # a workspace shorter than the slice: knn_graph walks in chunks, the same bytes
    index = ms._ready_index()
    short = index.byrows(64)
    # (handed out in place of the cache's: the cache itself would regrow a workspace shorter than the n ids knn_graph asks room for)
    real = ms._workspace_for
    ms._workspace_for = lambda kind, idx, need: short if kind == "byrows" else real(kind, idx, need)
    try:
        assert short.max_nq == 64 < world["n"]
        c_ids, c_scores = ms.knn_graph(K)
        assert c_ids.tobytes() == g_ids.tobytes() and c_scores.tobytes() == g_scores.tobytes()
    finally:
        del ms._workspace_for
        assert ms._workspace_for.__func__ is real.__func__
        short.close()
    # per-id filters, a TEXT_MATCH one among them; the same id under different filters; a band
    ids = np.array([3, 3, 3, 3, 3, 40, 41, 42, 43, 44, n - 1, 0], np.int64)
    per = [(FILTERS + [None])[i % 5] for i in range(len(ids))]
    for k in (1, K, 33):
        same(ms.search_by_ids(ids, k, filter=per), want(world, ids, k, per), ("per-id filters", k))
    lists = ms.search_by_ids(ids, K, filter=per, as_dicts=True)
    w = want(world, ids, K, per)
    code = [r["code"] for r in ms.client.records]
    assert [[h["code"] for h in hits] for hits in lists] == [[code[i] for i in row if i >= 0] for row in w[2]]
    assert [[h["score"] for h in hits] for hits in lists] == [[float(a) for a, i in zip(ra, ri) if i >= 0] for ra, ri in zip(w[0], w[2])]
    lo = float(world["fs"][3][30])
    same(ms.search_by_ids(ids, K, filter=per, radius=lo, range_filter=0.99), want(world, ids, K, per, radius=lo, range_filter=0.99), "a band")
    # similar_codes: the code's row, `search`'s dicts
    for r in (0, 17, n - 1):
        for e in (None, FILTERS[1], FILTERS[3]):
            hits = ms.similar_codes(code[r], K, filter=e)
            first = code.index(code[r])
            assert hits == ms.search_by_ids([first], K, filter=e, as_dicts=True)[0]
            assert [h["code"] for h in hits] == [code[i] for i in want(world, [first], K, [e])[2][0] if i >= 0] and code[r] not in [h["code"] for h in hits] or code.count(code[r]) > 1
    with pytest.raises(KeyError):
        ms.similar_codes("no-such-code", K)
    with pytest.raises(ValueError):
        ms.search_by_ids([n], K)


def test_the_batch_forms_equal_one_call_per_row_and_the_host_route(services, world):
    ms = services["ms"]
    assert ms.FILTER_ON_DEVICE and ms.TEXT_MATCH_ON_DEVICE
    ms._clear_views()
    check_routes(ms, world)
    assert not any("TEXT_MATCH" in f["expression"] for f in ms.filter_masks())   # the search's own masks were closed behind it


def test_the_same_with_the_masks_made_on_the_host(services, world):
    ms = services["ms"]
    ms._clear_views()
    ms.FILTER_ON_DEVICE = ms.TEXT_MATCH_ON_DEVICE = False
    try:
        check_routes(ms, world)
    finally:
        del ms.FILTER_ON_DEVICE, ms.TEXT_MATCH_ON_DEVICE
        ms._clear_views()


def test_endpoint(services, world):
    # (last of the module: the app's lifespan disconnects the installed services when the client closes)
    from fastapi.testclient import TestClient
    from rag_project_icd10_amd.api import app as appmod
    from rag_project_icd10_amd.services.multi_diagnosis_service import MultiDiagnosisService
    ms, es = services["ms"], services["es"]
    appmod.install_services(es, ms, MultiDiagnosisService(es, ms))
    try:
        with TestClient(appmod.app) as client:
            code = ms.client.records[17]["code"]
            for params, kw in (({"top_k": 5}, {}), ({"top_k": 7, "filter": FILTERS[3]}, {"filter": FILTERS[3]}), ({}, {})):
                r = client.get(f"/codes/{code}/similar", params=params)
                assert r.status_code == 200, r.text
                hits = ms.similar_codes(code, params.get("top_k", 10), **kw)
                cands = r.json()["candidates"]
                assert r.json()["code"] == code and len(hits) > 0
                assert [c["code"] for c in cands] == [h["code"] for h in hits]
                assert [(c["enhanced_score"], c["original_score"], c["title"]) for c in cands] == [(h["score"], h["original_score"], h["title"] or "") for h in hits]
                assert [(c["level"], c["parent_code"]) for c in cands] == [(h["metadata"]["level"], h["metadata"]["parent_code"]) for h in hits]
            assert client.get("/codes/no-such-code/similar").status_code == 404
            assert client.get(f"/codes/{code}/similar", params={"top_k": 0}).status_code == 400
            assert client.get(f"/codes/{code}/similar", params={"filter": "level =="}).status_code == 400
            assert client.get(f"/codes/{code}").status_code == 200
    finally:
        appmod.install_services(None, None, None)
