"""Range search, offset, iterator: everything that needs no GPU. The oracle walk (tests/range_oracle.py) against a brute force
over oracle.scores; the argument checks of icd_index_search_range, MilvusService and QueryRequest; the search_params spelling;
the iterator's bookkeeping against a stub index that answers from the oracle's ranking."""
import ctypes as C

import numpy as np
import pytest

from range_oracle import band_batch, band_query, in_band, pages

from rag_project_icd10_amd.services import range_search


def _brute(scores, levels, k, radius=None, range_filter=None, after=None, offset=0):
    """rules 1-3 and 7 by the book, one query: every row tested on its own, then ranked by (score desc, id asc)"""
    rows = []
    for i, s in enumerate(scores):
        s = np.float32(s)
        if np.isnan(s):
            continue
        if radius is not None and not s > np.float32(radius):
            continue
        if range_filter is not None and not s <= np.float32(range_filter):
            continue
        if after is not None:
            a_s, a_i = np.float32(after[0]), int(after[1])
            if not (s < a_s or (s.tobytes() == a_s.tobytes() and i > a_i)):
                continue
        rows.append(i)
    rows.sort(key=lambda i: (-float(scores[i]), i))
    return rows[offset:offset + k]


def test_oracle_walk_against_a_brute_force_over_the_oracle_scores(oracle):
    rng = np.random.default_rng(3)
    n, dim = 400, 32
    corpus = rng.standard_normal((n, dim)).astype(np.float32)
    corpus[1:60:2] = corpus[0:60:2]                     # exact duplicate pairs: score ties
    corpus[200] = np.nan                                # a row whose score is NaN is never a hit
    queries = np.concatenate([corpus[0:8:2], rng.standard_normal((4, dim)).astype(np.float32)])
    levels = rng.integers(1, 4, n).astype(np.int32)
    sc = np.stack([oracle.scores(q, corpus) for q in queries])
    ids = np.stack([np.array(sorted(range(n), key=lambda i: (np.isnan(r[i]), -float(r[i]) if not np.isnan(r[i]) else 0.0, i)), np.int64) for r in sc])
    ranked = np.take_along_axis(sc, ids, 1)
    for q in range(len(queries)):
        r = ranked[q]
        cases = [dict(), dict(radius=r[20]), dict(range_filter=r[20]), dict(radius=r[50], range_filter=r[10]), dict(radius=r[0]),
                 dict(after=(r[0], ids[q, 0])), dict(after=(r[1], ids[q, 1])), dict(after=(r[30], ids[q, 30]), radius=r[45]),
                 dict(after=(r[30], int(ids[q, 30]) + 1)), dict(after=(r[30], -5)), dict(range_filter=r[5], offset=3), dict(offset=390)]
        for case in cases:
            for k in (1, 10, 128):
                (raw, rid, lv), (adj, araw, aid, alv) = band_query(r, ids[q], levels, k, **case)
                want = _brute(sc[q], levels, k, **case)
                m = len(want)
                assert rid[:m].tolist() == want and (rid[m:] == -1).all(), (q, case, k)
                assert raw[:m].tobytes() == sc[q][want].tobytes() and np.isneginf(raw[m:]).all()
                assert lv[:m].tolist() == levels[want].tolist() and (lv[m:] == 0).all()
                w = {1: 1.2, 2: 1.0, 3: 0.8}
                a = [float(sc[q][i]) * w[int(levels[i])] for i in want]
                order = sorted(range(m), key=lambda j: -a[j])
                assert aid[:m].tolist() == [want[j] for j in order] and adj[:m].tolist() == [a[j] for j in order]
                assert (aid[m:] == -1).all() and np.isneginf(adj[m:]).all() and (alv[m:] == 0).all()
        # the twin of a duplicated row: first behind the lower id, gone behind the higher
        if q < 4:
            assert ids[q, 0] + 1 == ids[q, 1] and r[0].tobytes() == r[1].tobytes()
            assert band_query(r, ids[q], levels, 3, after=(r[0], ids[q, 0]))[0][1][0] == ids[q, 1]
            assert ids[q, 1] not in band_query(r, ids[q], levels, 128, after=(r[1], ids[q, 1]))[0][1]
        # pages: disjoint, their concatenation the band's ranking
        for bs, lim, b in ((7, -1, {}), (128, -1, {}), (16, 40, {}), (10, -1, dict(radius=r[95], range_filter=r[4]))):
            pg = pages(r, ids[q], bs, limit=lim, **b)
            flat = [i for p in pg for i in p]
            full = ids[q][in_band(r, ids[q], **b)].tolist()
            assert flat == (full if lim == -1 else full[:lim]) and all(len(p) == bs for p in pg[:-1])
    # a batch with per-query bounds
    lo = ranked[:, 30].copy()
    (raw, rid, lv), _adj = band_batch(ranked, ids, levels, 10, radius=lo)
    for q in range(len(queries)):
        assert rid[q].tolist() == _brute(sc[q], levels, 10, radius=lo[q])


def test_entry_point_argument_checks_need_no_device():
    from rag_project_icd10_amd import _native
    assert "icd_index_search_range" in _native.EXPORTED_SYMBOLS and hasattr(_native.IcdIndex, "search_range")
    lib = _native.load_library()
    assert lib.icd_abi_version() == 6
    q = np.zeros((2, 8), np.float32)
    adj, raw, ids = np.zeros((2, 10)), np.zeros((2, 10), np.float32), np.zeros((2, 10), np.int64)
    f32 = lambda *v: np.array(v, np.float32)

    def call(k=10, radius=None, range_filter=None, a_s=None, a_i=None, out_raw=raw, reweighted=1):
        p = lambda a: None if a is None else a.ctypes.data
        rc = lib.icd_index_search_range(None, q.ctypes.data, 2, k, 0, p(radius), p(range_filter), p(a_s), p(a_i), 0, reweighted,
                                        adj.ctypes.data, p(out_raw), ids.ctypes.data, None, 0, None)
        return rc, lib.icd_last_error().decode()
    for kw, text in ((dict(k=0), "k=0"), (dict(k=129), "k=129"), (dict(a_s=f32(1, 1)), "both or neither"),
                     (dict(a_i=np.zeros(2, np.int64)), "both or neither"), (dict(radius=f32(0.1, np.nan)), "radius[1] is NaN"),
                     (dict(range_filter=f32(np.nan, 1)), "range_filter[0] is NaN"),
                     (dict(a_s=f32(np.nan, 1), a_i=np.zeros(2, np.int64)), "after_scores[0] is NaN"),
                     (dict(radius=f32(0.1, 0.5), range_filter=f32(0.2, 0.5)), "query 1: radius=0.5"),
                     (dict(radius=f32(0.7, 0.1), range_filter=f32(0.2, 0.5)), "query 0: radius=0.7"), (dict(out_raw=None), "output pointer")):
        rc, msg = call(**kw)
        assert rc == -1 and text in msg, (kw, rc, msg)
    # good arguments get as far as the handle
    for kw in (dict(), dict(radius=f32(0.1, 0.2), range_filter=f32(0.2, 0.5)), dict(a_s=f32(1, 1), a_i=np.zeros(2, np.int64)),
               dict(radius=f32(-np.inf, 0.0), range_filter=f32(np.inf, np.inf)), dict(reweighted=0)):
        rc, msg = call(**kw)
        assert rc == -5 and "invalid handle" in msg, (kw, rc, msg)


def test_bounds_offset_and_search_params_rules():
    cb, co = range_search.check_bounds, range_search.check_offset
    assert cb() == (None, None) and cb(0.5) == (0.5, None) and cb(None, 1) == (None, 1.0) and cb(0.25, 0.5) == (0.25, 0.5)
    assert cb(search_params={"params": {"radius": 0.25, "range_filter": 0.5}}) == (0.25, 0.5)
    assert cb(search_params={"metric_type": "IP", "params": {"radius": 0.25}}) == (0.25, None)
    assert cb(search_params={"radius": 0.25}) == (0.25, None) and cb(search_params={"params": {}}) == (None, None)
    assert cb(0.25, search_params={"params": {"radius": 0.25, "range_filter": 0.5}}) == (0.25, 0.5)
    assert cb(np.float32(0.1))[0] == float(np.float32(0.1))       # the comparison runs on the fp32 score
    for bad in (dict(radius=0.5, range_filter=0.5), dict(radius=0.6, range_filter=0.5), dict(radius=float("nan")),
                dict(range_filter=float("nan")), dict(radius="0.5"), dict(radius=True), dict(search_params=[("radius", 1)]),
                dict(search_params={"params": 3}), dict(radius=0.1, search_params={"params": {"radius": 0.2}}),
                dict(search_params={"params": {"radius": 0.9, "range_filter": 0.1}})):
        with pytest.raises(ValueError):
            cb(**bad)
    assert co(0, 10) == 0 and co(16374, 10) == 16374 and co(np.int64(5), 1) == 5
    for bad in ((-1, 10), (16375, 10), (1.5, 10), ("3", 10), (True, 10)):
        with pytest.raises(ValueError):
            co(*bad)
    # MilvusService validates before it touches the store (no index, no GPU needed)
    from rag_project_icd10_amd.services.milvus_service import MilvusService
    ms = MilvusService.__new__(MilvusService)
    ms.client = None
    ms.collection_name = "none"
    q = np.zeros(8, np.float32)
    for kw in ({"radius": 0.5, "range_filter": 0.5}, {"radius": float("nan")}, {"offset": -1}, {"offset": 16380}, {"radius": "high"},
               {"radius": 0.1, "group_by_field": "level"}, {"range_filter": 0.1, "group_by_field": "level"}, {"offset": 2, "group_by_field": "level"},
               {"search_params": {"params": {"radius": 2, "range_filter": 1}}}):
        with pytest.raises(ValueError):
            ms.search(q, 5, **kw)
        with pytest.raises(ValueError):
            ms.search_batch(q[None], 5, **kw)
    for kw in ({"batch_size": 0}, {"batch_size": 129}, {"batch_size": 2.5}, {"limit": -2}, {"radius": 1.0, "range_filter": 0.5}, {"filter": "level >>"}):
        with pytest.raises(ValueError):
            ms.search_iterator(q, **kw)
    assert ms.search(q, 5, radius=0.1) == []                 # everything else keeps search's contract: logged, []
    it = ms.search_iterator(q, batch_size=5)                 # no collection: an iterator that is exhausted from the start
    assert it.next() == [] and it.close() is None


def test_query_request_range_fields_and_the_400():
    from pydantic import ValidationError
    from rag_project_icd10_amd.api.icd_models import QueryRequest
    r = QueryRequest(text="x")
    assert r.radius is None and r.range_filter is None
    r = QueryRequest(text="x", radius=0.5, range_filter=1)
    assert (r.radius, r.range_filter) == (0.5, 1.0)
    for bad in ({"radius": "high"}, {"range_filter": [1]}):
        with pytest.raises(ValidationError):
            QueryRequest(text="x", **bad)
    # a bad pair is the caller's error before any service is touched: 400 (no services installed here - a good pair is a 503)
    from fastapi.testclient import TestClient
    from rag_project_icd10_amd.api import app as appmod
    appmod.install_services(None, None, None)
    client = TestClient(appmod.app)
    assert client.post("/query", json={"text": "x", "radius": 0.5, "range_filter": 0.5}).status_code == 400
    assert client.post("/query", json={"text": "x", "radius": 0.7, "range_filter": 0.2}).status_code == 400
    assert client.post("/query", json={"text": "x", "radius": 0.2, "group_by_field": "level"}).status_code == 400
    assert client.post("/query", json={"text": "x", "radius": "high"}).status_code == 422
    assert client.post("/query", json={"text": "x", "radius": 0.2, "range_filter": 0.9}).status_code in (500, 503)


class _StubIndex:
    """answers search_range from a ranking, the way the device does: raw order, padded"""
    max_k, closed = 128, False

    def __init__(self, scores, ids, levels):
        self.s, self.i, self.levels, self.calls = scores, ids, levels, []

    def search_range(self, queries, k, *, radius=None, range_filter=None, after=None, reweighted=True):
        self.calls.append((k, after))
        raw, adj = band_batch(self.s, self.i, self.levels, k, radius, range_filter, after)
        return adj if reweighted else raw


def test_iterator_and_offset_bookkeeping_against_a_stub_index():
    rng = np.random.default_rng(9)
    n = 300
    sc = np.round(rng.standard_normal(n), 1).astype(np.float32)          # many ties
    ids = np.array(sorted(range(n), key=lambda i: (-float(sc[i]), i)), np.int64)
    ranked = sc[ids]
    levels = rng.integers(1, 4, n).astype(np.int32)
    gen = [0]
    to_hits = lambda adj, raw, i: [{"id": int(x), "score": float(a), "original_score": float(r)} for a, r, x in zip(adj, raw, i) if x >= 0]
    for bs, lim, b in ((7, -1, {}), (128, -1, {}), (16, 40, {}), (16, 48, {}), (10, -1, dict(radius=float(ranked[95]), range_filter=float(ranked[4]))), (5, 0, {})):
        stub = _StubIndex(ranked[None], ids[None], levels)
        it = range_search.SearchIterator(stub, np.zeros(4, np.float32), bs, lim, b.get("radius"), b.get("range_filter"), to_hits, lambda: gen[0])
        want = pages(ranked, ids, bs, b.get("radius"), b.get("range_filter"), limit=lim)
        seen = []
        for p, wp in enumerate(want):
            hits = it.next()
            assert it.last_raw_ids == wp and sorted(h["id"] for h in hits) == sorted(wp), (bs, lim, p)
            # the page is handed out re-sorted by adjusted score ...
            assert [h["score"] for h in hits] == sorted((h["score"] for h in hits), reverse=True)
            # ... but it was asked for behind the RAW-order last hit of the page before (that page's smallest key)
            _k, after = stub.calls[-1]
            if p == 0:
                assert after is None
            else:
                last = want[p - 1][-1]
                assert int(after[1]) == last and np.float32(after[0]).tobytes() == sc[last].tobytes()
            seen += wp
        assert it.next() == [] and it.next() == []
        flat = [i for w in want for i in w]
        assert seen == flat and len(set(flat)) == len(flat)
        if lim >= 0:
            assert len(flat) <= lim
        assert max((c[0] for c in stub.calls), default=0) <= bs
    # a changed store generation raises instead of paging through two corpora; a closed index too
    stub = _StubIndex(ranked[None], ids[None], levels)
    it = range_search.SearchIterator(stub, np.zeros(4, np.float32), 5, -1, None, None, to_hits, lambda: gen[0])
    assert len(it.next()) == 5
    gen[0] += 1
    with pytest.raises(RuntimeError):
        it.next()
    it.close()
    assert it.next() == []
    # offset: one search and a slice inside the page, cursor pages beyond it; always the reweight of exactly those k
    for o in (0, 7, 100, 128, 250, 295, 400):
        for k in (5, 28):
            stub = _StubIndex(ranked[None], ids[None], levels)
            got = range_search.search_band(stub, np.zeros((1, 4), np.float32), k, offset=o)
            want = band_batch(ranked[None], ids[None], levels, k, offset=o)[1]
            assert [np.asarray(g).tobytes() for g in got] == [w.tobytes() for w in want], (o, k)
            assert len(stub.calls) == (1 if o + k <= 128 else 1 + -(-o // 128))


@pytest.mark.parametrize("id_base", [1000, 2**32 + 12345])
def test_a_ranking_shifted_by_id_base_gives_the_same_outputs_with_the_ids_shifted(id_base):
    rng = np.random.default_rng(21)
    n, nq = 300, 5
    sc = np.round(rng.standard_normal((nq, n)), 1).astype(np.float32)   # many ties
    ids = np.stack([np.array(sorted(range(n), key=lambda i: (-float(r[i]), i)), np.int64) for r in sc])
    ranked = np.take_along_axis(sc, ids, 1)
    levels = rng.integers(1, 4, n).astype(np.int32)
    shift = lambda a: np.where(a >= 0, a + id_base, a)
    lo, hi = ranked[:, 120].copy(), ranked[:, 30].copy()
    cur = (ranked[:, 40].copy(), ids[:, 40].copy())
    below, above = (ranked[:, 40].copy(), np.full(nq, -3, np.int64)), (ranked[:, 40].copy(), np.full(nq, n + 7, np.int64))
    for case in (dict(), dict(radius=lo), dict(range_filter=hi), dict(radius=lo, range_filter=hi, after=cur), dict(after=cur, offset=3),
                 dict(after=below), dict(after=above)):
        for k in (1, 10, 128):
            want_raw, want_adj = band_batch(ranked, ids, levels, k, **case)
            moved = dict(case)
            if "after" in case:   # the cursor names a global id; one outside [0, n) lands outside [id_base, id_base + n) on the same side
                moved["after"] = (case["after"][0], case["after"][1] + id_base)
            got_raw, got_adj = band_batch(ranked, ids + id_base, levels, k, id_base=id_base, **moved)
            for j, (g, w) in enumerate(zip(got_raw + got_adj, want_raw + want_adj)):
                assert g.dtype == w.dtype and g.tobytes() == (shift(w) if w.dtype == np.int64 else w).tobytes(), (sorted(case), k, j)
    # the pages name their rows by the shifted ids
    assert pages(ranked[0], ids[0] + id_base, 7, radius=lo[0]) == [[i + id_base for i in p] for p in pages(ranked[0], ids[0], 7, radius=lo[0])]
