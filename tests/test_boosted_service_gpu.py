"""MilvusService.search_boosted / search_boosted_batch / search_boosted_iterator and POST /boosted_query on
the golden CSV slice's store, with the test encoder weights the neighbouring service tests use: every hit list against
tests/boost_oracle.py fed the STORED vectors and `filter_rows` of the same expressions - expression boosts, a TEXT_MATCH boost, a
per-query list of rankers, filters next to boosts, the masks made on the device and on the host. Exact: no tolerance."""
import os

import numpy as np
import pytest

import boost_oracle as bo

pytestmark = pytest.mark.gpu

from rag_project_icd10_amd.services.boost_ranker import BoostRanker  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EXPRS = ['level >= 2 and code like "A0%"', 'not (level == 1 or (code like "A01%" and not has_complication == true))',
         'parent_code != "" and (level in [2] or secondary_code like "G%")', 'TEXT_MATCH(preferred_zh, "伤寒")', "level >= 1"]
TEXTS = ["伤寒", "霍乱", "肺结核", "细菌性痢疾", "阿米巴病", "沙门菌感染", "急性心肌梗死"]


@pytest.fixture(scope="module")
def services(tmp_path_factory):
    mp = pytest.MonkeyPatch()
    mp.setenv("MILVUS_DB_PATH", str(tmp_path_factory.mktemp("db")))
    mp.setenv("MILVUS_COLLECTION_NAME", "icd10_boost")
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
    """the stored vectors, the queries, every query's canonical scores by row and every expression's rows, computed once"""
    ms, es = services["ms"], services["es"]
    corpus = np.ascontiguousarray(ms.client.matrix(), np.float32)
    levels = np.asarray(ms.client.levels(), np.int32)
    queries = np.ascontiguousarray(np.stack([np.asarray(es.encode_query(t), np.float32) for t in TEXTS]))
    by_row = np.stack([oracle.scores(q, corpus) for q in queries])
    keep = {e: np.isin(np.arange(len(corpus)), ms.filter_rows(e)) for e in EXPRS}
    assert all(0 < keep[e].sum() < len(corpus) for e in EXPRS[:4]) and keep[EXPRS[4]].all()
    return {"corpus": corpus, "levels": levels, "queries": queries, "by_row": by_row, "keep": keep}


def want_lists(world, top_k, per_query, filters, rows=None, **kw):
    """the oracle's reweighted lists as [(id, adjusted, boosted), ...] per query; per_query: lists of (expression, weight)"""
    rows = list(range(len(world["queries"]))) if rows is None else rows
    boosts = [[(world["keep"][e], w) for e, w in per] for per in per_query]
    _, rew = bo.boosted_batch(world["by_row"][rows], world["levels"], boosts, top_k, masks=[None if e is None else world["keep"][e] for e in filters], **kw)
    return [[(int(i), float(a), float(r)) for a, r, i in zip(rew[0][q], rew[1][q], rew[2][q]) if i >= 0] for q in range(len(rows))]


def got_lists(ms, lists):
    code_row = {r["code"]: i for i, r in enumerate(ms.client.records)}
    return [[(code_row[h["code"]], h["score"], h["original_score"]) for h in hits] for hits in lists]


def rankers(per):
    return [BoostRanker(e, w) for e, w in per]


def check_routes(ms, world):
    q = world["queries"]
    nq = len(q)
    f = lambda v: float(np.float32(v))   # noqa: E731
    shared = [(EXPRS[0], f(1.7)), (EXPRS[1], f(0.6))]
    text = [(EXPRS[3], f(2.5))]
    for top_k in (1, 10, 50):
        # one list of rankers for every query: expression boosts, and a TEXT_MATCH boost next to a filter
        assert got_lists(ms, ms.search_boosted_batch(q, top_k, rankers(shared), as_dicts=True)) == want_lists(world, top_k, [shared] * nq, [None] * nq)
        assert got_lists(ms, ms.search_boosted_batch(q, top_k, rankers(text), as_dicts=True, filter=EXPRS[2])) == want_lists(world, top_k, [text] * nq, [EXPRS[2]] * nq)
        # one list per query (none, one, four, a boost of every row), and one filter per query
        kinds = [[], text, [(EXPRS[0], f(1.7)), (EXPRS[1], f(0.6)), (EXPRS[2], f(1.2)), (EXPRS[3], f(3.0))], [(EXPRS[4], f(0.5))]]
        per = [kinds[i % 4] for i in range(nq)]
        filters = [(EXPRS[:3] + [None])[i % 4] for i in range(nq)]
        got = ms.search_boosted_batch(q, top_k, [rankers(p) if p else None for p in per], as_dicts=True, filter=filters)
        assert got_lists(ms, got) == want_lists(world, top_k, per, filters)
        # one query at a time; dict rankers; a band and an offset on the boosted score
        assert got_lists(ms, [ms.search_boosted(q[2], top_k, [{"filter": e, "weight": w} for e, w in shared], filter=EXPRS[2])]) == \
            want_lists(world, top_k, [shared], [EXPRS[2]], rows=[2])
    lo = float(np.sort(bo.boost_scores(world["by_row"][0], [(world["keep"][e], w) for e, w in shared]))[-30])
    assert got_lists(ms, [ms.search_boosted(q[0], 5, rankers(shared), radius=lo, offset=3)]) == want_lists(world, 5, [shared], [None], rows=[0], radius=lo, offset=3)
    # the arrays of a batch, and no boost at all: `search_batch` on the mask path
    adj, raw, ids, levels = ms.search_boosted_batch(q, 4, rankers(shared), filter='code like "A000%"')
    with np.errstate(invalid="ignore"):   # (padding is -inf behind -inf)
        assert ids.shape == (nq, 4) and (np.diff(adj, axis=1)[ids[:, 1:] >= 0] <= 0).all()
    plain = ms.search_batch(q, 10, filter=EXPRS[0], filter_mode="mask")
    assert all(a.tobytes() == b.tobytes() for a, b in zip(ms.search_boosted_batch(q, 10, None, filter=EXPRS[0]), plain))


def test_lists_equal_the_oracle_fed_the_stored_vectors(services, world):
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


def test_a_boost_reaches_below_the_plain_hit_list(services, world):
    """the TEXT_MATCH boost, its weight found from the oracle's scores so that the three best matching rows outrank every other
    row: a query whose plain top-10 holds fewer than three matching rows gets boosted hits `search` does not return at all"""
    ms = services["ms"]
    keep = world["keep"][EXPRS[3]]
    found = None
    for qi in range(len(world["queries"])):
        s = world["by_row"][qi]
        plain = set(np.argsort(-s.astype(np.float64), kind="stable")[:10].tolist())
        inside = np.nonzero(keep & (s > 0))[0]
        if len(inside) >= 3 and len(plain & set(inside.tolist())) < 3:
            third = np.sort(s[inside])[-3]
            found = (qi, float(np.float32(s[~keep].max() / third * 1.01)), plain)
            break
    assert found is not None
    qi, w, plain = found
    hits = ms.search_boosted(world["queries"][qi], 3, [BoostRanker(EXPRS[3], w)])
    assert got_lists(ms, [hits]) == want_lists(world, 3, [[(EXPRS[3], w)]], [None], rows=[qi])
    rows = [h[0] for h in got_lists(ms, [hits])[0]]
    assert len(rows) == 3 and keep[rows].all() and len(set(rows) - plain) >= 1


def test_iterator_pages_the_boosted_ranking(services, world):
    ms = services["ms"]
    per = [(EXPRS[0], float(np.float32(1.7))), (EXPRS[3], float(np.float32(2.5)))]
    boosts = [(world["keep"][e], w) for e, w in per]
    code_row = {r["code"]: i for i, r in enumerate(ms.client.records)}
    for flt, limit in ((None, 40), (EXPRS[2], -1)):
        want = bo.boosted_pages(world["by_row"][1], boosts, 7, mask=None if flt is None else world["keep"][flt], limit=limit)
        it = ms.search_boosted_iterator(world["queries"][1], rankers(per), batch_size=7, limit=limit, filter=flt)
        got = []
        while True:
            page = it.next()
            if not page:
                break
            assert sorted(code_row[h["code"]] for h in page) == sorted(it.last_raw_ids)
            got.append(list(it.last_raw_ids))
        it.close()
        assert got == want and len(got) > 3


def test_endpoint(services, world):
    # (last of the module: the app's lifespan disconnects the installed services when the client closes)
    from fastapi.testclient import TestClient
    from rag_project_icd10_amd.api import app as appmod
    from rag_project_icd10_amd.services.multi_diagnosis_service import MultiDiagnosisService
    ms, es = services["ms"], services["es"]
    per = [(EXPRS[0], float(np.float32(1.7))), (EXPRS[3], float(np.float32(2.5)))]
    appmod.install_services(es, ms, MultiDiagnosisService(es, ms))
    try:
        with TestClient(appmod.app) as client:
            r = client.post("/boosted_query", json={"texts": TEXTS[:3], "top_k": 5, "filter": EXPRS[2],
                                                    "boosts": [{"filter": e, "weight": w} for e, w in per]})
            assert r.status_code == 200, r.text
            body = r.json()
            service = ms.search_boosted_batch(world["queries"][:3], 5, rankers(per), as_dicts=True, filter=EXPRS[2])
            want = want_lists(world, 5, [per] * 3, [EXPRS[2]] * 3, rows=[0, 1, 2])
            assert got_lists(ms, service) == want
            for t, m in enumerate(body["diagnosis_matches"]):
                assert m["diagnosis_text"] == TEXTS[t]
                assert [c["code"] for c in m["candidates"]] == [ms.client.records[i]["code"] for i, _, _ in want[t]]
                assert [(c["enhanced_score"], c["original_score"]) for c in m["candidates"]] == [w[1:] for w in want[t]]
            assert body["candidates"] == body["diagnosis_matches"][0]["candidates"]
            assert client.post("/boosted_query", json={"texts": TEXTS[:1], "boosts": [{"filter": "level ==", "weight": 2.0}]}).status_code == 400
    finally:
        appmod.install_services(None, None, None)
