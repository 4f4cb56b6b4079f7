"""services/rank_of.py: RankOf.rank_of / rank_of_batch / evaluate over a MilvusService on the golden CSV slice's store, with the test encoder
weights the neighbouring service tests use: ranks, scores, levels and `selected` against tests/rankof_oracle.py over the CPU
oracle's full ranking - unfiltered, under a cached mask, a device filter program and a TEXT_MATCH, with the masks made on the
device and on the host; evaluate against the same metrics computed from the oracle's ranks; texts against their vectors; the API
route; an unknown code. Exact: no tolerance."""
import os

import numpy as np
import pytest

import rankof_oracle as ro

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILTERS = ['level >= 2 and code like "A0%"', 'not (level == 1 or (code like "A01%" and not has_complication == true))',
           'parent_code != "" and (level in [2] or secondary_code like "G%")', 'level >= 2 and TEXT_MATCH(preferred_zh, "伤寒")']
NQ = 40


@pytest.fixture(scope="module")
def services(tmp_path_factory):
    mp = pytest.MonkeyPatch()
    mp.setenv("MILVUS_DB_PATH", str(tmp_path_factory.mktemp("db")))
    mp.setenv("MILVUS_COLLECTION_NAME", "icd10_rankof")
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
    """the stored vectors, a fixed query batch, the oracle's full ranking of it, the filters' selections: computed once"""
    ms = services["ms"]
    corpus = np.ascontiguousarray(ms.client.matrix(), np.float32)
    levels = np.asarray(ms.client.levels(), np.int32)
    n = len(corpus)
    assert 100 <= n <= 300
    rng = np.random.default_rng(11)
    queries = np.ascontiguousarray(corpus[rng.integers(0, n, NQ)] + 0.05 * rng.standard_normal((NQ, corpus.shape[1])).astype(np.float32))
    fs, fi = oracle.flat_ip_topk(corpus, queries, n)
    keep = {e: None if e is None else np.isin(np.arange(n), ms.filter_rows(e)) for e in FILTERS + [None]}
    assert all(0 < keep[e].sum() < n for e in FILTERS)
    code = [r["code"] for r in ms.client.records]
    first = {}
    for i, c in enumerate(code):
        first.setdefault(c, i)
    return {"corpus": corpus, "levels": levels, "n": n, "queries": queries, "fs": fs, "fi": fi, "keep": keep, "code": code, "first": first}


def want_dicts(world, qsel, codes_per_query, filters):
    out = []
    for q, codes, e in zip(qsel, codes_per_query, filters):
        rows = np.array([world["first"][c] for c in codes], np.int64)
        rank, adj, raw, lv, sel = ro.rank_of_query(world["fs"][q], world["fi"][q], world["levels"], rows, world["keep"][e], world["n"])
        out.append([{"code": c, "rank": int(rank[j]) if rank[j] >= 0 else None, "score": float(adj[j]) if rank[j] >= 0 else None,
                     "raw_score": float(raw[j]) if rank[j] >= 0 else None, "level": int(lv[j]), "selected": sel} for j, c in enumerate(codes)])
    return out


def check_routes(ms, world):
    from rag_project_icd10_amd.services.rank_of import RankOf
    ranks = RankOf(ms)
    n, code, q = world["n"], world["code"], world["queries"]
    rng = np.random.default_rng(5)
    every = list(range(NQ))
    # ragged code lists (1 .. 16 codes, duplicates among them), unfiltered
    codes = [[code[r] for r in rng.integers(0, n, 1 + (i * 5) % 16)] for i in every]
    assert ranks.rank_of_batch(q, codes) == want_dicts(world, every, codes, [None] * NQ)
    # one filter for the batch: a scalar program (cached from then on), a TEXT_MATCH
    for e in (FILTERS[0], FILTERS[3]):
        got = ranks.rank_of_batch(q, codes, filter=e)
        assert got == want_dicts(world, every, codes, [e] * NQ), e
        assert any(h["rank"] is None for hits in got for h in hits)                # (codes the filter leaves out)
        assert ranks.rank_of_batch(q, codes, filter=e) == got                        # (the second call: the cached mask where there is one)
    # one filter per query, None among them
    per = [(FILTERS + [None])[i % 5] for i in every]
    assert ranks.rank_of_batch(q, codes, filter=per) == want_dicts(world, every, codes, per)
    # one query
    for i in (0, 7, NQ - 1):
        assert ranks.rank_of(q[i], codes[i], filter=per[i]) == want_dicts(world, [i], [codes[i]], [per[i]])[0]
        assert ranks.rank_of(q[i], codes[i][0]) == want_dicts(world, [i], [[codes[i][0]]], [None])[0]
    # evaluate: the best rank among the acceptable codes, from the oracle's ranks
    pairs = [(q[i], codes[i] if i % 2 else codes[i][0]) for i in every]
    for e in (None, FILTERS[1]):
        m = ranks.evaluate(pairs, ks=(1, 5, 10), filter=e)
        w = want_dicts(world, every, [p[1] if isinstance(p[1], list) else [p[1]] for p in pairs], [e] * NQ)
        best = [min([h["rank"] for h in hits if h["rank"] is not None], default=None) for hits in w]
        wm = ro.metrics(best)
        assert m["ranks"] == best and m["n"] == NQ
        for key in ("recall@1", "recall@5", "recall@10", "mrr", "mean_rank"):
            assert m[key] == pytest.approx(wm[key], rel=1e-12), key
    with pytest.raises(KeyError):
        ranks.rank_of(q[0], ["no-such-code"])
    with pytest.raises(KeyError):
        ranks.evaluate([(q[0], code[0]), (q[1], "no-such-code")])


def test_against_the_oracle(services, world):
    ms = services["ms"]
    assert ms.FILTER_ON_DEVICE and ms.TEXT_MATCH_ON_DEVICE
    ms._clear_views()
    check_routes(ms, world)
    assert not any("TEXT_MATCH" in f["expression"] for f in ms.filter_masks())   # the call's own masks were closed behind it


def test_the_same_with_the_masks_made_on_the_host(services, world):
    ms = services["ms"]
    ms._clear_views()
    ms.FILTER_ON_DEVICE = ms.TEXT_MATCH_ON_DEVICE = False
    try:
        check_routes(ms, world)
    finally:
        del ms.FILTER_ON_DEVICE, ms.TEXT_MATCH_ON_DEVICE
        ms._clear_views()


def test_texts_and_search_consistency(services, world):
    """a text is its encoded vector; the codes `search_batch` (mask mode, raw order aside) returns hold the ranks the raw list gives"""
    from rag_project_icd10_amd.services.rank_of import RankOf
    ms, es = services["ms"], services["es"]
    ranks = RankOf(ms)
    texts = [ms.client.records[r]["preferred_zh"] for r in (3, 50, 120)]
    vecs = np.asarray(es.encode_query_batch(texts), np.float32)
    codes = [[world["code"][3], world["code"][9]], [world["code"][50]], [world["code"][0], world["code"][120], world["code"][121]]]
    assert ranks.rank_of_batch(texts, codes, filter=FILTERS[2]) == ranks.rank_of_batch(vecs, codes, filter=FILTERS[2])
    assert ranks.rank_of(texts[1], codes[1]) == ranks.rank_of(vecs[1], codes[1])
    index = ms._ready_index()
    raw, ids, _lv = index.search_range(world["queries"], 16, reweighted=False)
    for i in (0, 5):
        hit_codes = [world["code"][r] for r in ids[i]]
        if len(set(hit_codes)) == len(hit_codes) and all(world["first"][c] == r for c, r in zip(hit_codes, ids[i])):
            got = ranks.rank_of(world["queries"][i], hit_codes)
            assert [h["rank"] for h in got] == list(range(16)) and [h["raw_score"] for h in got] == [float(s) for s in raw[i]]


def test_endpoint(services, world):
    # (last of the module: the app's lifespan disconnects the installed services when the client closes)
    from fastapi.testclient import TestClient
    from rag_project_icd10_amd.api import app as appmod
    from rag_project_icd10_amd.services.multi_diagnosis_service import MultiDiagnosisService
    from rag_project_icd10_amd.services.rank_of import RankOf
    ms, es = services["ms"], services["es"]
    ranks = RankOf(ms)
    appmod.install_services(es, ms, MultiDiagnosisService(es, ms))
    try:
        with TestClient(appmod.app) as client:
            text = ms.client.records[17]["preferred_zh"]
            codes = [world["code"][17], world["code"][3], world["code"][200]]
            for body, kw in (({"text": text, "codes": codes}, {}), ({"text": text, "codes": codes, "filter": FILTERS[3]}, {"filter": FILTERS[3]})):
                r = client.post("/codes/rank", json=body)
                assert r.status_code == 200, r.text
                assert r.json() == ranks.rank_of(text, codes, **kw)
            assert client.post("/codes/rank", json={"text": text, "codes": ["no-such-code"]}).status_code == 404
            assert client.post("/codes/rank", json={"text": text, "codes": []}).status_code == 400
            assert client.post("/codes/rank", json={"text": text, "codes": codes[:1] * 17}).status_code == 400
            assert client.post("/codes/rank", json={"text": text, "codes": codes, "filter": "level =="}).status_code == 400
    finally:
        appmod.install_services(None, None, None)
