"""MilvusService.search_mmr / search_mmr_batch on the golden CSV slice's store, with the test encoder
weights the neighbouring service tests use: every hit list against tests/mmr_oracle.py fed the STORED vectors, with no filter, one
filter and a list of filters, the filters' masks made on the device and on the host; lambda_mult = 1 against `search`; a query
whose diverse list spans more parent codes than its plain one, asserted as the oracle's exact list; the API route. Exact: no
tolerance."""
import os

import numpy as np
import pytest

from mmr_oracle import mmr_batch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILTERS = ['level >= 2 and code like "A0%"', 'not (level == 1 or (code like "A01%" and not has_complication == true))',
           'parent_code != "" and (level in [2] or secondary_code like "G%")', 'level >= 2 and TEXT_MATCH(preferred_zh, "伤寒")']
TEXTS = ["伤寒", "霍乱", "肺结核", "细菌性痢疾", "阿米巴病", "沙门菌感染", "急性心肌梗死"]


@pytest.fixture(scope="module")
def services(tmp_path_factory):
    mp = pytest.MonkeyPatch()
    mp.setenv("MILVUS_DB_PATH", str(tmp_path_factory.mktemp("db")))
    mp.setenv("MILVUS_COLLECTION_NAME", "icd10_mmr")
    mp.setenv("EMBEDDING_MODEL_NAME", "shibing624/text2vec-base-chinese")
    mp.setenv("ICD_EMBEDDING_ALLOW_SYNTHETIC", "1")
    from rag_project_icd10_amd.tools.build_database import DatabaseBuilder
    b = DatabaseBuilder()
    b.initialize_services()
    recs = b.load_csv_data(os.path.join(GOLDEN, "csv_slice.csv"))
    assert b.vectorize_and_index(recs) is True
    yield {"ms": b.milvus_service, "es": b.embedding_service}
    b.milvus_service.disconnect()
    mp.undo()


@pytest.fixture(scope="module")
def world(services, oracle):
    """the stored vectors, the queries and the oracle's full ranking of each, computed once"""
    ms, es = services["ms"], services["es"]
    corpus = np.ascontiguousarray(ms.client.matrix(), np.float32)
    levels = np.asarray(ms.client.levels(), np.int32)
    queries = np.ascontiguousarray(np.stack([np.asarray(es.encode_query(t), np.float32) for t in TEXTS]))
    fs, fi = oracle.flat_ip_topk(corpus, queries, len(corpus))
    keep = {e: None if e is None else np.isin(np.arange(len(corpus)), ms.filter_rows(e)) for e in FILTERS + [None]}
    assert all(0 < keep[e].sum() < len(corpus) for e in FILTERS)
    return {"corpus": corpus, "levels": levels, "queries": queries, "fs": fs, "fi": fi, "keep": keep}


def want_lists(oracle, world, top_k, fetch_k, lam, filters, rows=None, **bounds):
    """the oracle's reweighted lists as [(id, adjusted, raw, mmr), ...] per query"""
    rows = list(range(len(world["queries"]))) if rows is None else rows
    _, rew = mmr_batch(oracle, world["corpus"], world["levels"], world["fs"][rows], world["fi"][rows], top_k, fetch_k, lam,
                       masks=[world["keep"][e] for e in filters], **bounds)
    return [[(int(i), float(a), float(r), float(m)) for a, r, i, m in zip(rew[0][q], rew[1][q], rew[2][q], rew[4][q]) if i >= 0] for q in range(len(rows))]


def got_lists(ms, lists):
    code_row = {r["code"]: i for i, r in enumerate(ms.client.records)}
    return [[(code_row[h["code"]], h["score"], h["original_score"], h["mmr_score"]) for h in hits] for hits in lists]


def check_routes(ms, oracle, world):
    q = world["queries"]
    nq = len(q)
    cap = min(128, ms._ready_index().max_k)
    for top_k, fetch_k, lam in ((10, None, 0.5), (5, 40, 0.3), (3, 3, 0.0), (10, cap, 0.7)):
        fk = min(cap, max(20, 4 * top_k)) if fetch_k is None else fetch_k
        # no filter
        assert got_lists(ms, ms.search_mmr_batch(q, top_k, fetch_k, lam, as_dicts=True)) == want_lists(oracle, world, top_k, fk, lam, [None] * nq)
        # one filter for the whole batch, and through search_mmr one query at a time
        for e in FILTERS[:2] + FILTERS[3:]:
            want = want_lists(oracle, world, top_k, fk, lam, [e] * nq)
            assert got_lists(ms, ms.search_mmr_batch(q, top_k, fetch_k, lam, filter=e, as_dicts=True)) == want, e
            assert got_lists(ms, [ms.search_mmr(q[2], top_k, fetch_k, lam, filter=e)]) == want[2:3]
        # a list of filters, one entry per query
        per = [(FILTERS + [None])[i % 5] for i in range(nq)]
        assert got_lists(ms, ms.search_mmr_batch(q, top_k, fetch_k, lam, filter=per, as_dicts=True)) == want_lists(oracle, world, top_k, fk, lam, per)
    # a band shapes the candidate list
    lo = float(world["fs"][0][30])
    assert got_lists(ms, [ms.search_mmr(q[0], 5, 20, 0.5, radius=lo)]) == want_lists(oracle, world, 5, 20, 0.5, [None], rows=[0], radius=lo)
    # the arrays of a batch: adjusted-score order, padding behind the hits
    adj, raw, ids, levels, mmr = ms.search_mmr_batch(q, 4, 9, 0.5, filter='code like "A000%"')
    assert ids.shape == (nq, 4) and ((ids >= 0) == np.isfinite(mmr)).all() and (np.diff(adj, axis=1)[ids[:, 1:] >= 0] <= 0).all()


def test_lists_equal_the_oracle_fed_the_stored_vectors(services, oracle, world):
    ms = services["ms"]
    assert ms.FILTER_ON_DEVICE and ms.TEXT_MATCH_ON_DEVICE
    ms._clear_views()
    check_routes(ms, oracle, world)
    assert not any("TEXT_MATCH" in f["expression"] for f in ms.filter_masks())   # the search's own masks were closed behind it


def test_the_same_with_the_masks_made_on_the_host(services, oracle, world):
    ms = services["ms"]
    ms._clear_views()
    ms.FILTER_ON_DEVICE = ms.TEXT_MATCH_ON_DEVICE = False
    try:
        check_routes(ms, oracle, world)
    finally:
        del ms.FILTER_ON_DEVICE, ms.TEXT_MATCH_ON_DEVICE
        ms._clear_views()


def test_lambda_one_is_search(services, world):
    ms = services["ms"]
    for q in world["queries"]:
        for kw in ({}, {"filter": FILTERS[0]}, {"filter": FILTERS[2], "radius": -0.5}):
            plain = ms.search(q, 10, filter_mode="mask", **kw)
            diverse = ms.search_mmr(q, 10, 40, 1.0, **kw)
            assert [{k: v for k, v in h.items() if k != "mmr_score"} for h in diverse] == plain and len(plain) > 0
            assert [h["mmr_score"] for h in diverse] == [h["original_score"] for h in diverse]   # lambda 1: the value is the relevance


def test_a_diverse_list_spans_more_parents(services, oracle, world):
    """The query is chosen with the oracle alone, among the stored rows' own vectors: the one whose plain top-10 holds the fewest
    parent codes (one parent's children where the slice has such a query) and whose MMR list at lambda 0.5 holds more. The service
    must return the oracle's exact list."""
    ms = services["ms"]
    corpus, levels = world["corpus"], world["levels"]
    parent = [r.get("parent_code") or r["code"] for r in ms.client.records]
    fs, fi = oracle.flat_ip_topk(corpus, corpus, len(corpus))
    _, rew = mmr_batch(oracle, corpus, levels, fs, fi, 10, 40, 0.5)
    best = None
    for q in range(len(corpus)):
        plain = {parent[i] for i in fi[q][:10]}
        diverse = {parent[i] for i in rew[2][q] if i >= 0}
        if len(diverse) > len(plain) and (best is None or len(plain) < best[1]):
            best = (q, len(plain), len(diverse))
    assert best is not None, "no stored vector's diverse list spans more parents than its plain one"
    q = best[0]
    want = [(int(i), float(a), float(r), float(m)) for a, r, i, m in zip(rew[0][q], rew[1][q], rew[2][q], rew[4][q])]
    got = ms.search_mmr(corpus[q], 10, 40, 0.5)
    assert got_lists(ms, [got]) == [want]
    plain = ms.search(corpus[q], 10)
    assert len({h["metadata"]["parent_code"] or h["code"] for h in got}) == best[2] > best[1] == len({h["metadata"]["parent_code"] or h["code"] for h in plain})


def test_endpoint(services, oracle, world):
    # (last of the module: the app's lifespan disconnects the installed services when the client closes)
    from fastapi.testclient import TestClient
    from rag_project_icd10_amd.api import app as appmod
    from rag_project_icd10_amd.services.multi_diagnosis_service import MultiDiagnosisService
    ms, es = services["ms"], services["es"]
    appmod.install_services(es, ms, MultiDiagnosisService(es, ms))
    try:
        with TestClient(appmod.app) as client:
            r = client.post("/diverse_query", json={"text": TEXTS[0], "top_k": 5, "fetch_k": 30, "lambda_mult": 0.4, "filter": FILTERS[0]})
            assert r.status_code == 200, r.text
            want = want_lists(oracle, world, 5, 30, 0.4, [FILTERS[0]], rows=[0])[0]
            cands = r.json()["candidates"]
            assert [c["code"] for c in cands] == [ms.client.records[i]["code"] for i, _, _, _ in want]
            assert [(c["enhanced_score"], c["original_score"], c["similarity_factors"]["mmr_score"]) for c in cands] == [w[1:] for w in want]
            assert client.post("/diverse_query", json={"text": TEXTS[0], "top_k": 5, "fetch_k": 101}).status_code == 400   # above the store's max k
    finally:
        appmod.install_services(None, None, None)
