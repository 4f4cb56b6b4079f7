"""Grouping search (run with -m gpu on an MI355X): IcdIndex.search_grouped against a walk over the oracle's FULL ranking
(oracle.flat_ip_topk at k = n, tests/grouped_oracle.py), bit for bit; views, several groupings, graph capture, device tensors;
MilvusService / /query with group_by_field."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, icd_levels, unit_rows
from grouped_oracle import Ranking, expected

pytestmark = pytest.mark.gpu

from rag_project_icd10_amd import _native  # noqa: E402
from rag_project_icd10_amd._native import MODE_EXACT, IcdIndex  # noqa: E402

N = 12000
NQ = 300
KS = [(1, 1), (10, 1), (10, 3), (128, 1), (16, 8), (3, 40), (1, 128)]


def _bits(a):
    return np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a).tobytes()


def _corpus(kind):
    """the corpora of tests/test_filtered_search_gpu.py: exact duplicate pairs at rows 5000 + 2j / 5001 + 2j, queries = noisy
    copies of rows plus 40 of the duplicated rows themselves (exact ties)"""
    rng = np.random.default_rng({"gauss": 1, "family": 3, "aniso": 4}[kind])
    dim = 768
    if kind == "gauss":
        x = unit_rows(N, dim, 10 + len(kind), kind=kind)
    elif kind == "family":
        cent = rng.standard_normal((N // 120, dim)).astype(np.float32)
        x = np.repeat(cent, 120, axis=0) + 0.35 * rng.standard_normal((N, dim)).astype(np.float32)
    else:
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


def _groupings():
    """families of 120 rows (pairs start at even rows and 120 is even: every duplicate pair 5000 + 2j / 5001 + 2j shares a
    family); scattered (neighbouring rows land in different groups: every pair straddles two); three groups of 11 900 / 90 / 10
    rows in a seeded shuffle; identity; one group; 7 groups (fewer than k = 10: padding)"""
    rows = np.arange(N, dtype=np.int64)
    perm = np.random.default_rng(77).permutation(N)
    three = np.zeros(N, np.int64)
    three[perm[11900:11990]] = 1
    three[perm[11990:]] = 2
    return {"family": rows // 120, "scattered": (rows * 2654435761) % 37, "three": three, "identity": rows.copy(),
            "single": np.zeros(N, np.int64), "seven": rows % 7}


_CACHE = {}


def _parent(kind, oracle):
    if kind not in _CACHE:
        corpus, levels, q = _corpus(kind)
        s, i = oracle.flat_ip_topk(corpus, q, N)
        _CACHE[kind] = (corpus, levels, q, IcdIndex(corpus, levels, max_nq=NQ, max_k=128), s, i)
    return _CACHE[kind]


def _compare(got_raw, got_adj, want_raw, want_adj, what):
    names = ("raw", "ids", "levels", "groups")
    for name, g, w in zip(names, got_raw, want_raw):
        g = g.cpu().numpy() if hasattr(g, "cpu") else g
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype)
        assert _bits(g) == _bits(w), (what, "raw order", name, np.nonzero((g != w).any(1))[0][:5])
    for name, g, w in zip(("adj",) + names, got_adj, want_adj):
        g = g.cpu().numpy() if hasattr(g, "cpu") else g
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        assert _bits(g) == _bits(w), (what, "reweighted", name, np.nonzero((g != w).any(1))[0][:5])


def _distinct_groups_in_top128(ids, group_of):
    return np.array([len(set(group_of[row[:128]].tolist())) for row in ids])


@pytest.mark.parametrize("kind", ["gauss", "family", "aniso"])
def test_grouped_search_equals_the_walk_over_the_full_ranking(oracle, kind):
    corpus, levels, q, index, s_all, i_all = _parent(kind, oracle)
    dup_a, dup_b = np.arange(5000, 5400, 2), np.arange(5001, 5400, 2)
    for name, group_of in _groupings().items():
        if name == "family":
            assert (group_of[dup_a] == group_of[dup_b]).all()       # pairs that share a group ...
        if name == "scattered":
            assert (group_of[dup_a] != group_of[dup_b]).all()       # ... and pairs that straddle two
        rk = Ranking(s_all, i_all, group_of)
        if kind == "family" and name in ("family", "three"):
            # the condition that keeps this test honest: a de-duplicated top-128 cannot answer these
            kk = 10 if name == "family" else 3
            short = (_distinct_groups_in_top128(i_all, group_of) < kk).mean()
            print(f"{kind}/{name}: {100 * short:.1f} % of the queries have fewer than {kk} groups in their top-128")
            assert short >= 0.90, (name, short)
        grouping = index.grouping(group_of)
        st = grouping.stats()
        assert st["groups"] == len(np.unique(group_of)) and st["largest_group"] == np.bincount(group_of).max() and st["bytes"] > 0
        for k, s in KS:
            want_raw, want_adj = expected(oracle, rk, levels, k, s)
            if name == "seven" and k == 10:
                assert (want_raw[1][:, 7 * s:] == -1).all() and (want_raw[3][:, 7 * s:] == -1).all()
            for nq in (NQ, 1, 4, 17):
                got_raw = index.search_grouped(q[:nq], k, s, grouping, reweighted=False)
                got_adj = index.search_grouped(q[:nq], k, s, grouping, reweighted=True)
                _compare(got_raw, got_adj, tuple(w[:nq] for w in want_raw), tuple(w[:nq] for w in want_adj), (kind, name, k, s, nq))
            if name == "identity" and s == 1:     # rule 5: every row its own group = the plain search
                ps, pi = index.search(q, k, MODE_EXACT)
                a, r, i, lv = index.search_reweighted(q, k, MODE_EXACT)
                g_raw = index.search_grouped(q, k, 1, grouping, reweighted=False)
                g_adj = index.search_grouped(q, k, 1, grouping, reweighted=True)
                assert _bits(g_raw[0]) == _bits(ps) and _bits(g_raw[1]) == _bits(pi)
                assert _bits(g_adj[0]) == _bits(a) and _bits(g_adj[1]) == _bits(r) and _bits(g_adj[2]) == _bits(i) and _bits(g_adj[3]) == _bits(lv)
            if name == "single" and k == 1:       # rule 5: one group, group_size m = the plain search at k = m
                ps, pi = index.search(q, s, MODE_EXACT)
                g_raw = index.search_grouped(q, 1, s, grouping, reweighted=False)
                assert _bits(g_raw[0]) == _bits(ps) and _bits(g_raw[1]) == _bits(pi)
        grouping.close()


@pytest.mark.parametrize("sel", ["half", "154"])
def test_grouped_search_on_a_view(oracle, sel):
    corpus, levels, q, index, _s, _i = _parent("family", oracle)
    rng = np.random.default_rng(11)
    rows = np.sort(rng.choice(N, N // 2 if sel == "half" else 154, replace=False)).astype(np.int64)
    view = index.view(rows)
    vs, vi = oracle.flat_ip_topk(corpus[rows], q, len(rows))
    for name in ("family", "scattered", "three"):
        group_of = _groupings()[name][rows]
        rk = Ranking(vs, vi, group_of)
        grouping = view.grouping(group_of)
        for k, s in ((10, 1), (10, 3), (3, 40)):
            want_raw, want_adj = expected(oracle, rk, levels, k, s, row_map=rows)
            got_raw = view.search_grouped(q, k, s, grouping, reweighted=False)
            got_adj = view.search_grouped(q, k, s, grouping, reweighted=True)
            _compare(got_raw, got_adj, want_raw, want_adj, (sel, name, k, s))
        grouping.close()
    view.close()


def test_two_groupings_device_tensors_capture_and_lifetimes(oracle):
    import torch
    corpus, levels, q, index, s_all, i_all = _parent("gauss", oracle)
    gs = _groupings()
    ga, gb = index.grouping(gs["family"]), index.grouping(torch.from_numpy(gs["scattered"]).cuda())
    wa = expected(oracle, Ranking(s_all, i_all, gs["family"]), levels, 10, 3)
    wb = expected(oracle, Ranking(s_all, i_all, gs["scattered"]), levels, 10, 3)
    dq = torch.from_numpy(q).cuda()
    for _ in range(2):   # interleaved: the two groupings do not disturb each other
        for grouping, (want_raw, want_adj) in ((ga, wa), (gb, wb)):
            got_raw = index.search_grouped(dq, 10, 3, grouping, reweighted=False)
            got_adj = index.search_grouped(dq, 10, 3, grouping, reweighted=True)
            assert all(t.is_cuda for t in got_raw + got_adj)
            _compare(got_raw, got_adj, want_raw, want_adj, "device")
    # a grouped search inside a graph replays to the same bits (one single-branch graph, default queue settings)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        index.search_grouped(dq, 10, 3, ga)   # warm-up on the capture stream
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        cap = index.search_grouped(dq, 10, 3, ga)
    for _ in range(2):
        for t in cap:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for g, w in zip(cap, wa[1]):
            assert _bits(g) == _bits(w)
    del graph
    # a grouping of another index, a closed grouping, bad k / group_size
    other = IcdIndex(corpus[:256], levels[:256], max_nq=8, max_k=10)
    go = other.grouping(np.arange(256) % 5)
    with pytest.raises(_native.IcdError) as e:
        index.search_grouped(q[:2], 3, 1, go)
    assert e.value.code == -1
    for k, s in ((0, 1), (1, 0), (129, 1), (16, 9), (1, 129)):
        with pytest.raises(ValueError, match="128"):
            index.search_grouped(q[:2], k, s, ga)
    with pytest.raises(ValueError):
        index.grouping(np.arange(N) - 1)
    with pytest.raises(ValueError):
        index.grouping(np.arange(N - 1))
    # either may go first
    other.close()
    go.close()
    gb.close()
    ga.close()
    with pytest.raises(_native.IcdError):
        index.search_grouped(q[:2], 3, 1, ga)
    tmp = IcdIndex(corpus[:512], levels[:512], max_nq=8, max_k=10)
    gt = tmp.grouping(np.arange(512) // 8)
    r = tmp.search_grouped(q[:3], 4, 2, gt, reweighted=False)
    gt.close()
    tmp.close()
    assert (r[1] >= 0).all()


# ---- services ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def services(tmp_path_factory):
    mp = pytest.MonkeyPatch()
    mp.setenv("MILVUS_DB_PATH", str(tmp_path_factory.mktemp("db")))
    mp.setenv("MILVUS_COLLECTION_NAME", "icd10_grouped")
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


def _field_values(recs, field):
    if field == "category":
        return [(r.get("category_path") or "").split(">")[0].strip() or r["code"] for r in recs]
    if field == "level":
        return [int(r.get("level", 1)) for r in recs]
    return ["" if r.get(field) is None else str(r.get(field)) for r in recs]


def _field_groups(recs, field):
    vals = _field_values(recs, field)
    rank = {v: i for i, v in enumerate(sorted(set(vals)))}
    return np.array([rank[v] for v in vals], np.int64), vals


PLAIN_KEYS = {"code", "title", "score", "original_score", "metadata"}
PLAIN_META = {"has_complication", "main_code", "secondary_code", "level", "parent_code", "category_path", "semantic_text"}


@pytest.mark.parametrize("expr", [None, 'code like "A0%"', "level >= 2"])
@pytest.mark.parametrize("field", ["parent_code", "level", "category"])
def test_milvus_service_group_by_field(services, oracle, field, expr):
    ms, es, recs = services["ms"], services["es"], services["recs"]
    corpus, levels = ms.client.matrix(), ms.client.levels()
    rows = np.arange(len(recs), dtype=np.int64) if expr is None else ms.filter_rows(expr)
    group_all, vals = _field_groups(recs, field)
    vecs = np.stack([es.encode_query(s) for s in services["strings"]]).astype(np.float32)
    s_all, i_all = oracle.flat_ip_topk(corpus[rows], vecs, len(rows))
    rk = Ranking(s_all, i_all, group_all[rows])
    for k, gs in ((1, 1), (5, 1), (5, 3), (3, 20)):
        _raw, (adj, raw, ids, lv, grp) = expected(oracle, rk, levels, k, gs, row_map=rows)
        kw = {} if expr is None else {"filter": expr}
        batch = ms.search_batch(vecs, k, as_dicts=True, group_by_field=field, group_size=gs, **kw)
        arrays = ms.search_batch(vecs, k, group_by_field=field, group_size=gs, **kw)
        assert len(arrays) == 5 and _bits(arrays[2]) == _bits(ids) and _bits(arrays[0]) == _bits(adj) and _bits(arrays[4]) == _bits(grp)
        for q in range(len(vecs)):
            hits = batch[q]
            m = int((ids[q] >= 0).sum())
            assert [h["code"] for h in hits] == [recs[i]["code"] for i in ids[q, :m]], (field, expr, k, gs, q)
            assert [h["score"] for h in hits] == [float(a) for a in adj[q, :m]]
            assert [h["original_score"] for h in hits] == [float(r) for r in raw[q, :m]]
            assert [h["metadata"][field] for h in hits] == [vals[i] for i in ids[q, :m]]
            assert len({h["metadata"][field] for h in hits}) <= k
            if q < 6:
                assert ms.search(vecs[q], k, group_by_field=field, group_size=gs, **kw) == hits
    # without the new arguments a hit has the shape it had: no new key
    for h in ms.search(vecs[0], 5) + ms.search_batch(vecs[:2], 5, as_dicts=True)[1]:
        assert set(h) == PLAIN_KEYS and set(h["metadata"]) == PLAIN_META
    assert len(ms.search_batch(vecs, 5)) == 4
    cached = ms.groupings()
    assert any(g["field"] == field and g["groups"] == len(set(np.asarray(vals, dtype=object)[rows].tolist())) and g["bytes"] > 0 for g in cached), cached
    for bad in ({"group_by_field": "nope"}, {"group_by_field": field, "group_size": 0}, {"group_by_field": field, "group_size": 26},
                {"group_size": 2}):
        with pytest.raises(ValueError):
            ms.search(vecs[0], 5, **bad)
        with pytest.raises(ValueError):
            ms.search_batch(vecs, 5, **bad)


def test_groupings_dropped_with_the_store(services):
    ms, es, recs = services["ms"], services["es"], list(services["recs"])
    vec = es.encode_query(recs[3]["semantic_text"])
    before = ms.search(vec, 4, group_by_field="category", group_size=2)
    assert before and ms.groupings()
    mat = ms.client.matrix().copy()
    order = np.arange(len(recs))[::-1]
    assert ms.clear_collection() and not ms.groupings()
    assert ms.insert_records([recs[i] for i in order], [mat[i] for i in order])
    after = ms.search(vec, 4, group_by_field="category", group_size=2)
    assert sorted(h["code"] for h in after) == sorted(h["code"] for h in before)
    assert ms.clear_collection() and ms.insert_records(recs, [mat[i] for i in range(len(recs))])


def test_match_diagnoses_batch_grouped_equals_one_at_a_time(services):
    from rag_project_icd10_amd.services.multi_diagnosis_service import MultiDiagnosisService
    ms, es, strings = services["ms"], services["es"], services["strings"]
    md = MultiDiagnosisService(es, ms)
    for field, gs in (("category", 1), ("parent_code", 2)):
        batched = md.match_diagnoses_batch(strings, top_k=3, group_by_field=field, group_size=gs)
        for i, d in enumerate(strings):
            hits = ms.search(es.encode_query(d), 6, group_by_field=field, group_size=gs)
            one = md._match_from_hits(d, hits, 3)
            assert batched[i].model_dump() == one.model_dump(), (field, gs, d)


def test_query_endpoint_with_group_by_field(services):
    # (last of the module: the app's lifespan disconnects the installed services when the client closes)
    from fastapi.testclient import TestClient
    from rag_project_icd10_amd.api import app as appmod
    from rag_project_icd10_amd.services.multi_diagnosis_service import MultiDiagnosisService
    ms, es, recs = services["ms"], services["es"], services["recs"]
    appmod.install_services(es, ms, MultiDiagnosisService(es, ms))
    cat = dict(zip((r["code"] for r in recs), _field_values(recs, "category")))
    try:
        with TestClient(appmod.app) as client:
            text = "霍乱，伤寒；副伤寒"
            plain = client.post("/query", json={"text": text, "top_k": 3})
            assert plain.status_code == 200 and plain.json()["candidates"]
            r = client.post("/query", json={"text": text, "top_k": 3, "group_by_field": "category"})
            body = r.json()
            assert r.status_code == 200 and body["candidates"], body
            for m in body["diagnosis_matches"]:   # one row per category: the candidates of a diagnosis are of distinct categories
                cats = [cat[c["code"]] for c in m["candidates"]]
                assert len(cats) == len(set(cats)) == 3, cats
            r2 = client.post("/query", json={"text": text, "top_k": 3, "group_by_field": "category", "group_size": 2, "filter": "level >= 2"})
            assert r2.status_code == 200 and r2.json()["candidates"]
            assert client.post("/query", json={"text": text, "group_by_field": "nope"}).status_code == 400
            assert client.post("/query", json={"text": text, "top_k": 50, "group_by_field": "level", "group_size": 2}).status_code == 400
            assert client.post("/query", json={"text": text, "group_size": 2}).status_code == 400
            assert client.post("/query", json={"text": text, "group_by_field": "level", "group_size": 0}).status_code == 422
            stats = client.get("/stats").json()
            assert any(g["field"] == "category" and g["groups"] > 0 for g in stats["groupings"]), stats
            assert client.post("/query", json={"text": text, "top_k": 3}).json() == plain.json()
    finally:
        appmod.install_services(None, None, None)
