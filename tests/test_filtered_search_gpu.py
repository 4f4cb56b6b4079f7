"""Filtered search (run with -m gpu on an MI355X): views of an index (icd_index_create_view) against the oracle over the selected
rows, bit for bit; MilvusService / MultiDiagnosisService / /query with a Milvus `filter` expression against the unfiltered
machinery run on the selection."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, icd_levels, unit_rows

pytestmark = pytest.mark.gpu

from rag_project_icd10_amd import _native  # noqa: E402
from rag_project_icd10_amd._native import MODE_AUTO, MODE_EXACT, IcdIndex  # noqa: E402

N = 12000
NQ = 300
KS = [1, 10, 32, 64, 100, 128]


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _corpus(kind):
    """rows of four shapes, with exact duplicate pairs (rows 5000 + 2j and 5001 + 2j) whose copies a selection may split; queries
    are noisy copies of rows plus the duplicated rows themselves (exact ties)"""
    rng = np.random.default_rng({"gauss": 1, "clustered": 2, "family": 3, "aniso": 4}[kind])
    dim = 768
    if kind in ("gauss", "clustered"):
        x = unit_rows(N, dim, 10 + len(kind), kind=kind)
    elif kind == "family":   # families of 120 near-identical rows in code order
        cent = rng.standard_normal((N // 120, dim)).astype(np.float32)
        x = np.repeat(cent, 120, axis=0) + 0.35 * rng.standard_normal((N, dim)).astype(np.float32)
    else:                    # a large common component: cosine of two rows ~0.96 (the fp16 image is centred)
        mu = rng.standard_normal(dim).astype(np.float32)
        x = mu / np.linalg.norm(mu) + (0.2 / np.sqrt(dim)) * rng.standard_normal((N, dim)).astype(np.float32)
    x = np.asarray(x, np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    x[5001:5400:2] = x[5000:5400:2]
    x = np.ascontiguousarray(x, dtype=np.float32)
    src = rng.integers(0, N, NQ - 40)
    q = x[src] + 0.05 * rng.standard_normal((NQ - 40, dim)).astype(np.float32)
    q = np.concatenate([x[5000:5080:2], q]).astype(np.float32)
    return x, icd_levels(N, 7), np.ascontiguousarray(q)


_CACHE = {}


def _parent(kind):
    if kind not in _CACHE:
        corpus, levels, q = _corpus(kind)
        _CACHE[kind] = (corpus, levels, q, IcdIndex(corpus, levels, max_nq=NQ, max_k=128))
    return _CACHE[kind]


def _selections(k, seed):
    rng = np.random.default_rng(seed)
    out = {}
    for size in (1, k - 1, k, 37, 1000, N // 2, N - 1, N):
        if size >= 1:
            out[size] = np.sort(rng.choice(N, size, replace=False)).astype(np.int64)
    # a selection that holds one copy of every duplicate pair and not the other
    out["split_pairs"] = np.sort(np.concatenate([np.arange(5000, 5400, 2), rng.choice(np.arange(5400, N), 3000, replace=False)]))
    return out


def _expected(oracle, corpus, levels, q, rows, k):
    s, i = oracle.flat_ip_topk(corpus[rows], q, k)
    gid = np.where(i >= 0, rows[np.clip(i, 0, None)], -1)
    return oracle.reweight(s, gid, levels)


def _check(got, want, what):
    adj, raw, ids, lv = (t.cpu().numpy() if hasattr(t, "cpu") else t for t in got)
    assert np.array_equal(ids, want[2]), (what, np.nonzero((ids != want[2]).any(1))[0][:5])
    assert _bits(adj) == _bits(want[0]) and _bits(raw) == _bits(want[1]) and np.array_equal(lv, want[3]), what


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("kind", ["gauss", "clustered", "family", "aniso"])
def test_view_equals_the_oracle_over_the_selected_rows(oracle, kind, k):
    """ids (the parent's), raw, adj and levels of a view, bit for bit the oracle's top-k over corpus[rows] mapped through rows
    and reweighted with the parent's levels - selections of 1, k - 1, k, 37, 1 000, half, all but one and all rows, batches
    of 1 / 4 / 16 / 300 queries, AUTO and EXACT; short selections are padded with id -1"""
    corpus, levels, q, parent = _parent(kind)
    for name, rows in _selections(k, 100 + k).items():
        view = parent.view(rows)
        assert view.n == len(rows) and view.stats()["n"] == len(rows)
        want = _expected(oracle, corpus, levels, q, rows, k)
        if len(rows) < k:
            assert (want[2][:, len(rows):] == -1).all()
        for nq in (1, 4, 16, NQ):
            for mode in (MODE_AUTO, MODE_EXACT):
                got = view.search_reweighted(q[:nq], k, mode)
                _check(got, tuple(w[:nq] for w in want), (kind, k, name, nq, mode))
        if name == "split_pairs":   # the kept copy of a duplicate pair is found at its own id, never the excluded one's
            ids = want[2][:40]
            assert all(5000 + 2 * j in ids[j] for j in range(40)) and not np.isin(ids[:40], np.arange(5001, 5400, 2)).any()
        view.close()


def test_full_selection_gives_the_parents_outputs(oracle):
    corpus, levels, q, parent = _parent("gauss")
    view = parent.view(np.arange(N))
    for k in (10, 100):
        for nq in (1, 16, NQ):
            a, b = parent.search_reweighted(q[:nq], k), view.search_reweighted(q[:nq], k)
            for x, y in zip(a, b):
                assert _bits(x) == _bits(y), (k, nq)
            s1, i1 = parent.search(q[:nq], k)
            s2, i2 = view.search(q[:nq], k)
            assert np.array_equal(i1, i2) and _bits(s1) == _bits(s2)
    view.close()


def test_view_device_tensors_and_independent_lifetime(oracle):
    """device-in / device-out calls (torch CUDA rows and queries), raw search ids, and a view that outlives its parent"""
    import torch
    corpus, levels, q = _corpus("clustered")
    parent = IcdIndex(torch.from_numpy(corpus).cuda(), levels, max_nq=NQ, max_k=64)
    rows = np.sort(np.random.default_rng(5).choice(N, 4321, replace=False)).astype(np.int64)
    view = parent.view(torch.from_numpy(rows).cuda())
    assert np.array_equal(view.rows, rows)
    parent.close()
    for k in (10, 64):
        want = _expected(oracle, corpus, levels, q, rows, k)
        dq = torch.from_numpy(q).cuda()
        got = view.search_reweighted(dq, k)
        assert all(t.is_cuda for t in got)
        _check(got, want, ("device", k))
        _check(view.search_reweighted(q, k), want, ("host", k))
        s, i = view.search(dq, k)
        os_, oi = oracle.flat_ip_topk(corpus[rows], q, k)
        assert np.array_equal(i.cpu().numpy(), rows[oi]) and _bits(s.cpu().numpy()) == _bits(os_)
    view.close()


def test_large_batch_on_a_view(oracle):
    """10 000 queries (the view's own probe runs: max_nq >= 2 048) at k = 10, AUTO and EXACT"""
    corpus, levels, q, parent = _parent("family")
    rng = np.random.default_rng(9)
    qb = corpus[rng.integers(0, N, 10000)] + 0.05 * rng.standard_normal((10000, corpus.shape[1])).astype(np.float32)
    qb = np.ascontiguousarray(qb, dtype=np.float32)
    for rows in (np.sort(rng.choice(N, N // 2, replace=False)), np.delete(np.arange(N), 777)):
        view = parent.view(rows.astype(np.int64), max_nq=10000, max_k=10)
        want = _expected(oracle, corpus, levels, qb, rows, 10)
        for mode in (MODE_AUTO, MODE_EXACT):
            _check(view.search_reweighted(qb, 10, mode), want, ("10k", len(rows), mode))
        view.close()


def test_view_argument_errors():
    corpus, levels, q, parent = _parent("gauss")
    for bad in ([], [3, 3], [5, 4], [-1, 2], [0, N]):
        with pytest.raises(_native.IcdError) as e:
            parent.view(np.asarray(bad, np.int64))
        assert e.value.code == -1, bad
    view = parent.view(np.arange(0, N, 7))
    import torch
    with pytest.raises(_native.IcdError) as e:
        view.lookup_levels(torch.zeros(4, dtype=torch.int64, device="cuda"))
    assert e.value.code == -4
    with pytest.raises(_native.IcdError) as e:
        _native.IcdGroup(view, _native.GROUP_ROW_SHARD)
    assert e.value.code == -4
    st = view.stats()
    assert st["n"] == len(range(0, N, 7)) and st["bytes_corpus_f32"] == st["n"] * 768 * 4
    view.close()


# ---- services ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def services(tmp_path_factory):
    mp = pytest.MonkeyPatch()
    mp.setenv("MILVUS_DB_PATH", str(tmp_path_factory.mktemp("db")))
    mp.setenv("MILVUS_COLLECTION_NAME", "icd10_filter")
    mp.setenv("EMBEDDING_MODEL_NAME", "shibing624/text2vec-base-chinese")
    mp.setenv("ICD_EMBEDDING_ALLOW_SYNTHETIC", "1")
    from rag_project_icd10_amd.tools.build_database import DatabaseBuilder
    b = DatabaseBuilder()
    b.initialize_services()
    recs = b.load_csv_data(os.path.join(GOLDEN, "csv_slice.csv"))
    assert b.vectorize_and_index(recs) is True
    strings = [l.rstrip("\n") for l in open(os.path.join(GOLDEN, "diagnosis_strings.txt"), encoding="utf-8")][:40]
    yield {"b": b, "recs": recs, "ms": b.milvus_service, "es": b.embedding_service, "strings": strings}
    b.milvus_service.disconnect()
    mp.undo()


EXPRS = ['code like "A0%"', "level >= 2", 'code like "%.9"', 'level == 1 or code in ["A01.0", "A02.1"]',
         'not code like "A%"', 'code == "A00"', "level > 0", 'code == "none"']


def test_milvus_search_with_filter_matches_the_reference_shape(services, oracle):
    from rag_project_icd10_amd.services import filter_expr
    ms, es, recs = services["ms"], services["es"], services["recs"]
    corpus, levels = ms.client.matrix(), ms.client.levels()
    for expr in EXPRS:
        rows = ms.filter_rows(expr)
        want_rows = filter_expr.select(expr, filter_expr.Columns.from_records(recs))
        assert np.array_equal(rows, want_rows), expr
        for s in services["strings"][:12]:
            vec = es.encode_query(s)
            for k in (1, 5, 20):
                hits = ms.search(vec, k, filter=expr)
                if len(rows) == 0:
                    assert hits == []
                    continue
                want = oracle.reference_shaped_search(corpus[rows], levels[rows], vec, k)
                assert [h["code"] for h in hits] == [recs[rows[i]]["code"] for _a, _b, i in want], (expr, s, k)
                assert max(abs(h["score"] - a) for h, (a, _b, _i) in zip(hits, want)) <= 1e-5
                assert max(abs(h["original_score"] - b) for h, (_a, b, _i) in zip(hits, want)) <= 1e-5
            # search_batch(..., filter) == search once per query
        vecs = np.stack([es.encode_query(s) for s in services["strings"]])
        batch = ms.search_batch(vecs, 5, as_dicts=True, filter=expr)
        assert batch == [ms.search(v, 5, filter=expr) for v in vecs], expr
        adj, raw, ids, lv = ms.search_batch(vecs, 5, filter=expr)
        assert np.isin(ids[ids >= 0], rows).all() and ((ids >= 0).sum(1) == min(5, len(rows))).all()
    # the whole corpus selected: the parent itself; the cache holds the views made above, at most ICD_FILTER_VIEWS of them
    views = ms.filter_views()
    assert 0 < len(views) <= 8 and all(v["rows"] < len(recs) and v["bytes"] > 0 for v in views)
    assert ms.search(es.encode_query("霍乱"), 5, filter="level > 0") == ms.search(es.encode_query("霍乱"), 5)
    assert ms.search(es.encode_query("霍乱"), 5, filter="level >") == []
    with pytest.raises(ValueError):
        ms.search_batch(vecs, 5, filter="level >")


@pytest.mark.parametrize("with_entities", [False, True])
def test_match_diagnoses_batch_with_filter_equals_one_at_a_time(services, with_entities):
    from test_entity_rescoring_cpu import synthetic_entities
    from rag_project_icd10_amd.services.multi_diagnosis_service import MultiDiagnosisService
    ms, es, strings = services["ms"], services["es"], services["strings"]
    md = MultiDiagnosisService(es, ms)
    ents = [synthetic_entities(i, s) for i, s in enumerate(strings)] if with_entities else None
    for expr in ('code like "A0%"', "level >= 2", 'code == "none"'):
        allowed = {services["recs"][i]["code"] for i in ms.filter_rows(expr)}
        for k in (3, 5):
            batched = md.match_diagnoses_batch(strings, top_k=k, entities=ents, filter=expr)
            for i, d in enumerate(strings):
                hits = ms.search(es.encode_query(d), 2 * k, filter=expr)
                one = md._match_from_hits(d, hits, k, ents[i]) if with_entities else md._match_from_hits(d, hits, k)
                assert batched[i].model_dump() == one.model_dump(), (expr, d, k)
                assert {c.code for c in batched[i].candidates} <= allowed
    # the request API: device path and host path pass the filter alike
    res = md.match_multiple_diagnoses("霍乱，伤寒；副伤寒", top_k=3, filter='code like "A0%"')
    allowed = {services["recs"][i]["code"] for i in ms.filter_rows('code like "A0%"')}
    assert res["matches"] and all(c.code in allowed for m in res["matches"] for c in m.candidates)
    ms.supports_device_rescoring = lambda: False
    try:
        host = md.match_multiple_diagnoses("霍乱，伤寒；副伤寒", top_k=3, filter='code like "A0%"')
    finally:
        del ms.supports_device_rescoring
    assert [m.model_dump() for m in host["matches"]] == [m.model_dump() for m in res["matches"]]


def test_stale_views_after_a_rebuild_with_the_same_row_count(services):
    """clear + insert the same number of rows in another order: a filtered search answers from the NEW rows (the cache is keyed
    on the store's generation, not on its row count)"""
    ms, es, recs = services["ms"], services["es"], list(services["recs"])
    vec = es.encode_query(recs[3]["semantic_text"])
    expr = 'code like "A0%"'
    before = ms.search(vec, 5, filter=expr)
    assert before and len(ms.filter_views()) > 0
    mat = ms.client.matrix().copy()
    order = np.arange(len(recs))[::-1]
    # the rebuilt store holds the same rows reversed, and every title marked: a stale view would return old ids / titles
    new_recs = [dict(recs[i], preferred_zh="新" + (recs[i].get("preferred_zh") or "")) for i in order]
    assert ms.clear_collection() and not ms.filter_views()
    assert ms.insert_records(new_recs, [mat[i] for i in order])
    assert ms.client.count == len(recs)
    after = ms.search(vec, 5, filter=expr)
    assert sorted(h["code"] for h in after) == sorted(h["code"] for h in before)
    assert all(h["title"].startswith("新") for h in after)
    rows = ms.filter_rows(expr)
    assert all(ms.client.records[i]["code"].startswith("A0") for i in rows)
    # restore the fixture's store for any later test
    assert ms.clear_collection() and ms.insert_records(recs, [mat[i] for i in range(len(recs))])


def test_query_endpoint_with_filter(services):
    # (last of the module: the app's lifespan disconnects the installed services when the client closes)
    from fastapi.testclient import TestClient
    from rag_project_icd10_amd.api import app as appmod
    from rag_project_icd10_amd.services.multi_diagnosis_service import MultiDiagnosisService
    ms, es = services["ms"], services["es"]
    appmod.install_services(es, ms, MultiDiagnosisService(es, ms))
    try:
        with TestClient(appmod.app) as client:
            plain = client.post("/query", json={"text": "霍乱，伤寒；副伤寒", "top_k": 3})
            assert plain.status_code == 200 and plain.json()["candidates"]
            r = client.post("/query", json={"text": "霍乱，伤寒；副伤寒", "top_k": 3, "filter": "level >= 2"})
            allowed = {services["recs"][i]["code"] for i in ms.filter_rows("level >= 2")}
            body = r.json()
            assert r.status_code == 200 and body["candidates"], body
            assert all(c["code"] in allowed for m in body["diagnosis_matches"] for c in m["candidates"])
            assert client.post("/query", json={"text": "霍乱", "filter": "level == 'x'"}).status_code == 400
            stats = client.get("/stats").json()
            assert any(v["expression"] == "level >= 2" for v in stats["filter_views"]), stats
            # no filter: the same response as before the filtered calls
            assert client.post("/query", json={"text": "霍乱，伤寒；副伤寒", "top_k": 3}).json() == plain.json()
    finally:
        appmod.install_services(None, None, None)
