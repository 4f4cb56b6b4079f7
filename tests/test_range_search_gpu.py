"""Range search, offset and the search iterator (run with -m gpu on an MI355X): IcdIndex.search_range against a walk over the
oracle's FULL ranking (oracle.flat_ip_topk at k = n, tests/range_oracle.py), bit for bit. The bounds of every case are taken
per query FROM that ranking, so every case is decided by construction. Corpora: those of tests/test_grouped_search_gpu.py."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from range_oracle import band_batch, pages
from test_grouped_search_gpu import N, NQ, _corpus

pytestmark = pytest.mark.gpu

from rag_project_icd10_amd import _native  # noqa: E402
from rag_project_icd10_amd._native import MODE_EXACT, IcdIndex  # noqa: E402
from rag_project_icd10_amd.services import range_search  # noqa: E402

BATCHES = (1, 2, 4, 40, NQ)   # single-launch form (1, 2, 4), sparse streaming form (40), fp32-MFMA form (300)
_CACHE = {}


def _bits(a):
    return np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a).tobytes()


def _parent(kind, oracle):
    if kind not in _CACHE:
        corpus, levels, q = _corpus(kind)
        s, i = oracle.flat_ip_topk(corpus, q, N)
        _CACHE[kind] = (corpus, levels, q, IcdIndex(corpus, levels, max_nq=NQ, max_k=128), s, i)
    return _CACHE[kind]


def _cut(v, nq):
    if v is None:
        return None
    if isinstance(v, tuple):
        return tuple(_cut(x, nq) for x in v)
    return v[:nq] if hasattr(v, "__len__") else v


def _check(index, q, want, k, nq, what, **bounds):
    """search_range of the first nq queries, raw and reweighted, against the first nq rows of `want` (band_batch's result)"""
    b = {name: _cut(v, nq) for name, v in bounds.items()}
    got_raw = index.search_range(q[:nq], k, reweighted=False, **b)
    got_adj = index.search_range(q[:nq], k, reweighted=True, **b)
    for label, got, exp in (("raw", got_raw, want[0]), ("reweighted", got_adj, want[1])):
        assert len(got) == len(exp)
        for j, (g, w) in enumerate(zip(got, exp)):
            g = g.cpu().numpy() if hasattr(g, "cpu") else g
            w = w[:nq]
            assert g.dtype == w.dtype and g.shape == w.shape, (what, label, j, g.dtype, w.dtype, g.shape, w.shape)
            assert _bits(g) == _bits(w), (what, label, j, nq, k, np.nonzero((g != w).any(1))[0][:5])


@pytest.mark.parametrize("kind", ["gauss", "family", "aniso"])
def test_hits_under_a_ceiling_lie_beyond_the_top_128(oracle, kind):
    corpus, levels, q, index, s_all, i_all = _parent(kind, oracle)
    ceiling = s_all[:, 200].copy()
    for k in (1, 10, 100, 128):
        want = band_batch(s_all, i_all, levels, k, range_filter=ceiling)
        # the condition that keeps a post-filter of the ordinary search from passing: no expected hit is in the plain top-128
        share = np.mean([len(set(want[0][1][r][want[0][1][r] >= 0].tolist()) & set(i_all[r, :128].tolist())) > 0 for r in range(NQ)])
        print(f"{kind} k={k}: {100 * share:.1f} % of the queries have an expected hit inside the plain top-128")
        assert share == 0.0
        assert (want[0][1] >= 0).all()
        for nq in BATCHES:
            _check(index, q, want, k, nq, (kind, "ceiling"), range_filter=ceiling)


@pytest.mark.parametrize("kind", ["gauss", "family", "aniso"])
def test_floor_both_bounds_empty_band_and_no_bound(oracle, kind):
    corpus, levels, q, index, s_all, i_all = _parent(kind, oracle)
    for r in (0, 5, 127, 500):
        floor = s_all[:, r].copy()
        for k in (10, 128):
            want = band_batch(s_all, i_all, levels, k, radius=floor)
            n_hits = (want[0][1] >= 0).sum(1)
            assert (n_hits <= min(r, k)).all()           # the row AT the floor is out: at most r rows lie above it ...
            assert (n_hits == min(r, k)).mean() > 0.8    # ... and exactly r where the score at rank r is not tied with rank r - 1
            for nq in BATCHES:
                _check(index, q, want, k, nq, (kind, "floor", r), radius=floor)
    # both bounds: the row AT range_filter is in, the row AT radius is out
    lo, hi = s_all[:, 300].copy(), s_all[:, 150].copy()
    assert (lo < hi).all()
    for k in (10, 100):
        want = band_batch(s_all, i_all, levels, k, radius=lo, range_filter=hi)
        assert (want[0][1][:, 0] == i_all[np.arange(NQ), [int(np.nonzero(s_all[r] <= hi[r])[0][0]) for r in range(NQ)]]).all()
        for nq in BATCHES:
            _check(index, q, want, k, nq, (kind, "both"), radius=lo, range_filter=hi)
    # different kinds of bounds per query in one batch: no bound / floor only / ceiling only / both
    lo2 = np.where(np.arange(NQ) % 4 == 1, s_all[:, 40], np.where(np.arange(NQ) % 4 == 3, s_all[:, 260], -np.inf)).astype(np.float32)
    hi2 = np.where(np.arange(NQ) % 4 >= 2, s_all[:, 180], np.inf).astype(np.float32)
    want = band_batch(s_all, i_all, levels, 100, radius=lo2, range_filter=hi2)
    for nq in BATCHES:
        _check(index, q, want, 100, nq, (kind, "mixed"), radius=lo2, range_filter=hi2)
    # an empty band: all padding
    top = s_all[:, 0].copy()
    want = band_batch(s_all, i_all, levels, 10, radius=top)
    assert (want[0][1] == -1).all() and np.isneginf(want[1][0]).all()
    for nq in BATCHES:
        _check(index, q, want, 10, nq, (kind, "empty"), radius=top)
    _check(index, q, want, 10, NQ, (kind, "empty scalar"), radius=10.0)
    # rule 6: no bound at all = the MODE_EXACT search, bit for bit
    for k in (10, 128):
        for nq in BATCHES:
            ps, pi = index.search(q[:nq], k, MODE_EXACT)
            a, r, i, lv = index.search_reweighted(q[:nq], k, MODE_EXACT)
            g_raw = index.search_range(q[:nq], k, reweighted=False)
            g_adj = index.search_range(q[:nq], k)
            assert _bits(g_raw[0]) == _bits(ps) and _bits(g_raw[1]) == _bits(pi)
            assert [_bits(t) for t in g_adj] == [_bits(t) for t in (a, r, i, lv)]


@pytest.mark.parametrize("kind", ["gauss", "family"])
def test_cursor_on_each_member_of_a_duplicate_pair(oracle, kind):
    corpus, levels, q, index, s_all, i_all = _parent(kind, oracle)
    # queries 0 .. 39 ARE rows 5000 + 2 j, whose twin is row 5001 + 2 j: the two best hits tie exactly, lower id first
    pair = np.arange(40)
    assert (i_all[pair, 0] == 5000 + 2 * pair).all() and (i_all[pair, 1] == 5001 + 2 * pair).all()
    assert _bits(s_all[pair, 0]) == _bits(s_all[pair, 1])
    for member in (0, 1):
        after = (s_all[:, member].copy(), i_all[:, member].copy())
        for k in (10, 128):
            want = band_batch(s_all, i_all, levels, k, after=after)
            if member == 0:
                assert (want[0][1][pair, 0] == 5001 + 2 * pair).all()     # the twin is the first hit behind the lower id ...
            else:
                assert not (want[0][1][pair] == 5001 + 2 * pair[:, None]).any() and (want[0][1][pair, 0] == i_all[pair, 2]).all()   # ... and gone behind the higher
            for nq in BATCHES:
                _check(index, q, want, k, nq, (kind, "after", member), after=after)
    # cursors on rows of EVERY position inside a 128-row tile (a tile's rows sit in different registers and lanes of the MFMA form):
    # query r's cursor is the best of its 400 best hits whose id is r modulo 128 (rank 0 when there is none)
    ranks = np.array([next((j for j in range(400) if i_all[r, j] % 128 == r % 128), 0) for r in range(NQ)])
    assert len(set((i_all[np.arange(NQ), ranks] % 128).tolist())) >= 100
    after = (s_all[np.arange(NQ), ranks].copy(), i_all[np.arange(NQ), ranks].copy())
    for k in (10, 100):
        want = band_batch(s_all, i_all, levels, k, after=after)
        for nq in (40, NQ):
            _check(index, q, want, k, nq, (kind, "after, every tile position"), after=after)
    # cursor and bounds together, deep in the ranking
    after = (s_all[:, 700].copy(), i_all[:, 700].copy())
    want = band_batch(s_all, i_all, levels, 100, radius=s_all[:, 760].copy(), after=after)
    assert ((want[0][1] >= 0).sum(1) <= 59).all()
    for nq in BATCHES:
        _check(index, q, want, 100, nq, (kind, "after + floor"), radius=s_all[:, 760].copy(), after=after)


def test_range_search_on_a_view_with_a_cursor_outside_it(oracle):
    corpus, levels, q, index, _s, _i = _parent("family", oracle)
    rng = np.random.default_rng(11)
    rows = np.sort(rng.choice(N, N // 2, replace=False)).astype(np.int64)
    inside = set(rows.tolist())
    view = index.view(rows)
    vs, vi = oracle.flat_ip_topk(corpus[rows], q, len(rows))
    gi = rows[vi]                                            # the view's hits carry the parent's ids
    ceiling = vs[:, 200].copy()
    for k in (10, 128):
        want = band_batch(vs, gi, levels, k, range_filter=ceiling)
        for nq in BATCHES:
            _check(view, q, want, k, nq, ("view", "ceiling"), range_filter=ceiling)
    # a cursor that names a row OUTSIDE the view (the next id above hit 50 that the view does not hold) with hit 50's score
    out_ids = []
    for r in range(NQ):
        c = int(gi[r, 50]) + 1
        while c in inside:
            c += 1
        out_ids.append(c)
    after = (vs[:, 50].copy(), np.array(out_ids, np.int64))
    want = band_batch(vs, gi, levels, 10, after=after)
    for nq in BATCHES:
        _check(view, q, want, 10, nq, ("view", "after outside"), after=after)
    after_in = (vs[:, 50].copy(), gi[:, 50].copy())
    want = band_batch(vs, gi, levels, 100, after=after_in)
    assert (want[0][1][:, 0] == gi[:, 51]).all()
    for nq in (1, 40, NQ):
        _check(view, q, want, 100, nq, ("view", "after inside"), after=after_in)
    view.close()


def test_device_tensors_and_graph_capture(oracle):
    import torch
    corpus, levels, q, index, s_all, i_all = _parent("gauss", oracle)
    dq = torch.from_numpy(q).cuda()
    lo, hi = s_all[:, 300].copy(), s_all[:, 150].copy()
    after = (s_all[:, 170].copy(), i_all[:, 170].copy())
    dev = lambda a: torch.from_numpy(a).cuda()
    for k in (10, 100):
        want = band_batch(s_all, i_all, levels, k, radius=lo, range_filter=hi, after=after)
        for nq in BATCHES:
            b = {"radius": dev(lo[:nq]), "range_filter": dev(hi[:nq]), "after": (dev(after[0][:nq]), dev(after[1][:nq]))}
            got = index.search_range(dq[:nq], k, **b)
            assert all(t.is_cuda for t in got)
            _check(index, dq, want, k, nq, ("device", k), radius=dev(lo), range_filter=dev(hi), after=(dev(after[0]), dev(after[1])))
    # one device-in / device-out call inside a graph replays to the same bits (single-branch graph, no runtime setting touched)
    want = band_batch(s_all, i_all, levels, 10, radius=lo, range_filter=hi, after=after)
    for nq in (1, 40, NQ):
        b = {"radius": dev(lo[:nq]), "range_filter": dev(hi[:nq]), "after": (dev(after[0][:nq]), dev(after[1][:nq]))}
        qs = dq[:nq].contiguous()
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            index.search_range(qs, 10, **b)   # warm-up on the capture stream
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            cap = index.search_range(qs, 10, **b)
        for _ in range(2):
            for t in cap:
                t.zero_()
            graph.replay()
            torch.cuda.synchronize()
            for g, w in zip(cap, want[1]):
                assert _bits(g) == _bits(w[:nq]), nq
        del graph
    # argument errors of the binding and the entry point
    with pytest.raises(ValueError):
        index.search_range(q[:2], 0)
    with pytest.raises(ValueError):
        index.search_range(q[:2], 10, after=(s_all[:2, 0], None))
    with pytest.raises(ValueError):
        index.search_range(q[:3], 10, radius=np.zeros(2, np.float32))
    for bad in ({"radius": 0.5, "range_filter": 0.5}, {"radius": 0.6, "range_filter": 0.5}, {"radius": float("nan")},
                {"range_filter": float("nan")}, {"after": (np.full(2, np.nan, np.float32), np.zeros(2, np.int64))}):
        with pytest.raises(_native.IcdError) as e:
            index.search_range(q[:2], 10, **bad)
        assert e.value.code == -1, bad


def test_pages_concatenate_to_the_full_ranking_and_offsets_are_its_slices(oracle):
    corpus, levels, q, index, s_all, i_all = _parent("family", oracle)
    sel = np.r_[0:4, 100:104]     # four queries that are duplicated rows, four ordinary ones
    qs, ss, ii = q[sel], s_all[sel], i_all[sel]
    got_s, got_i, after = [], [], None
    for _page in range((N + 127) // 128 + 1):
        raw, ids, _lv = index.search_range(qs, 128, after=after, reweighted=False)
        if (ids < 0).all():
            break
        got_s.append(raw)
        got_i.append(ids)
        valid = (ids >= 0).sum(1)
        assert (valid == valid[0]).all()
        if valid[0] < 128:
            break
        after = (raw[:, -1].copy(), ids[:, -1].copy())
    got_s, got_i = np.concatenate(got_s, 1), np.concatenate(got_i, 1)
    assert len(got_s[0]) >= N and (got_i[:, N:] == -1).all()
    assert _bits(got_i[:, :N]) == _bits(ii) and _bits(got_s[:, :N]) == _bits(ss)
    # ONE query, pages of 10 (the single-launch form), 30 pages deep
    want_pages = pages(ss[0], ii[0], 10, limit=300)
    after = None
    for p in range(30):
        raw, ids, _lv = index.search_range(qs[0], 10, after=after, reweighted=False)
        assert ids[0].tolist() == want_pages[p], p
        after = (raw[:, -1].copy(), ids[:, -1].copy())
    # offset: ranks o .. o + k of the ranking in raw order, THEN the reweight and re-sort of those k
    for o in (0, 7, 128, 1000):
        for k in (10, 100):
            want = band_batch(ss, ii, levels, k, offset=o)
            got = range_search.search_band(index, qs, k, offset=o)
            assert [_bits(g) for g in got] == [_bits(w) for w in want[1]], (o, k)
        want = band_batch(ss, ii, levels, 10, range_filter=ss[:, 200].copy(), offset=o)
        for r in range(len(sel)):     # (the service layer takes ONE band per call)
            got = range_search.search_band(index, qs[r:r + 1], 10, range_filter=float(ss[r, 200]), offset=o)
            assert [_bits(g) for g in got] == [_bits(w[r:r + 1]) for w in want[1]], (o, r)


# ---- services ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def services(tmp_path_factory):
    mp = pytest.MonkeyPatch()
    mp.setenv("MILVUS_DB_PATH", str(tmp_path_factory.mktemp("db")))
    mp.setenv("MILVUS_COLLECTION_NAME", "icd10_range")
    mp.setenv("EMBEDDING_MODEL_NAME", "shibing624/text2vec-base-chinese")
    mp.setenv("ICD_EMBEDDING_ALLOW_SYNTHETIC", "1")
    from rag_project_icd10_amd.tools.build_database import DatabaseBuilder
    b = DatabaseBuilder()
    b.initialize_services()
    recs = b.load_csv_data(os.path.join(GOLDEN, "csv_slice.csv"))
    assert b.vectorize_and_index(recs) is True
    strings = [l.rstrip("\n") for l in open(os.path.join(GOLDEN, "diagnosis_strings.txt"), encoding="utf-8")][:12]
    yield {"b": b, "recs": recs, "ms": b.milvus_service, "es": b.embedding_service, "strings": strings}
    b.milvus_service.disconnect()
    mp.undo()


@pytest.mark.parametrize("expr", [None, "level >= 2"])
def test_milvus_service_radius_offset_and_iterator(services, oracle, expr):
    ms, es, recs = services["ms"], services["es"], services["recs"]
    corpus, levels = ms.client.matrix(), ms.client.levels()
    rows = np.arange(len(recs), dtype=np.int64) if expr is None else ms.filter_rows(expr)
    vecs = np.stack([es.encode_query(s) for s in services["strings"]]).astype(np.float32)
    s_all, i_loc = oracle.flat_ip_topk(corpus[rows], vecs, len(rows))
    i_all = rows[i_loc]
    kw = {} if expr is None else {"filter": expr}
    codes = lambda ids: [recs[i]["code"] for i in ids if i >= 0]
    for qi in range(len(vecs)):
        floor, ceil = float(s_all[qi, 12]), float(s_all[qi, 3])
        for k, o, b in ((5, 0, {"radius": floor}), (20, 0, {"radius": floor}), (5, 0, {"radius": floor, "range_filter": ceil}),
                        (5, 0, {"range_filter": ceil}), (5, 4, {}), (5, 4, {"radius": floor}), (10, 95, {}), (10, 130, {"range_filter": ceil})):
            _raw, (adj, raw, ids, lv) = band_batch(s_all[qi:qi + 1], i_all[qi:qi + 1], levels, k, b.get("radius"), b.get("range_filter"), offset=o)
            hits = ms.search(vecs[qi], k, offset=o, **b, **kw)
            m = int((ids[0] >= 0).sum())
            assert [h["code"] for h in hits] == codes(ids[0]) and len(hits) == m, (qi, k, o, b)
            assert [h["score"] for h in hits] == [float(a) for a in adj[0, :m]]
            assert [h["original_score"] for h in hits] == [float(r) for r in raw[0, :m]]
            if "radius" in b:
                assert all(h["original_score"] > np.float32(floor) for h in hits)
        # Milvus's spelling
        assert ms.search(vecs[qi], 5, search_params={"params": {"radius": floor, "range_filter": ceil}}, **kw) == \
            ms.search(vecs[qi], 5, radius=floor, range_filter=ceil, **kw)
    # search_batch: one band for the whole batch; arrays and dicts
    floor = float(np.median(s_all[:, 8]))
    _raw, want = band_batch(s_all, i_all, levels, 10, radius=floor)
    arrays = ms.search_batch(vecs, 10, radius=floor, **kw)
    assert [_bits(a) for a in arrays] == [_bits(w) for w in want]
    dicts = ms.search_batch(vecs, 10, as_dicts=True, radius=floor, **kw)
    assert [[h["code"] for h in d] for d in dicts] == [codes(r) for r in want[2]]
    _raw, want = band_batch(s_all, i_all, levels, 10, radius=floor, offset=3)
    assert [_bits(a) for a in ms.search_batch(vecs, 10, radius=floor, offset=3, **kw)] == [_bits(w) for w in want]
    # the iterator: disjoint pages, raw-order concatenation = the band's ranking, limit, exhaustion
    for qi in (0, 5):
        for bs, lim, b in ((7, -1, {}), (16, 40, {}), (100, -1, {"radius": float(s_all[qi, 150])}), (10, -1, {"radius": float(s_all[qi, 25]), "range_filter": float(s_all[qi, 2])})):
            want_pages = pages(s_all[qi], i_all[qi], bs, b.get("radius"), b.get("range_filter"), limit=lim)
            it = ms.search_iterator(vecs[qi], batch_size=bs, limit=lim, **b, **kw)
            seen = []
            for p, wp in enumerate(want_pages):
                hits = it.next()
                assert it.last_raw_ids == wp, (qi, bs, p)
                assert sorted(h["code"] for h in hits) == sorted(codes(wp))
                assert [h["score"] for h in hits] == sorted((h["score"] for h in hits), reverse=True)
                seen += wp
            assert it.next() == [] and it.next() == []
            assert len(seen) == len(set(seen))
            it.close()
    # a mutation of the store under an iterator
    it = ms.search_iterator(vecs[0], batch_size=5, **kw)
    assert len(it.next()) == 5
    mat = ms.client.matrix().copy()
    assert ms.clear_collection() and ms.insert_records(list(recs), [mat[i] for i in range(len(recs))])
    with pytest.raises(RuntimeError):
        it.next()
    for bad in ({"radius": 0.5, "range_filter": 0.5}, {"radius": float("nan")}, {"offset": -1}, {"offset": 16380}, {"radius": "high"},
                {"radius": 0.1, "group_by_field": "level"}, {"offset": 2, "group_by_field": "level"}):
        with pytest.raises(ValueError):
            ms.search(vecs[0], 5, **bad)
        with pytest.raises(ValueError):
            ms.search_batch(vecs, 5, **bad)


def test_match_diagnoses_and_query_endpoint_with_radius(services):
    # (last of the module: the app's lifespan disconnects the installed services when the client closes)
    from fastapi.testclient import TestClient
    from rag_project_icd10_amd.api import app as appmod
    from rag_project_icd10_amd.services.multi_diagnosis_service import MultiDiagnosisService
    ms, es, strings = services["ms"], services["es"], services["strings"]
    md = MultiDiagnosisService(es, ms)
    vec = es.encode_query(strings[0])
    plain = ms.search(vec, 10)
    floor = plain[4]["original_score"] if len(plain) > 4 else 0.0
    # the device rescoring path takes the padded lists of a narrow band: batch = one at a time
    raws = sorted((h["original_score"] for h in plain), reverse=True)
    floor = float(raws[3])
    batched = md.match_diagnoses_batch(strings, top_k=3, radius=floor)
    for i, d in enumerate(strings):
        hits = ms.search(es.encode_query(d), 6, radius=floor)
        assert all(h["original_score"] > np.float32(floor) for h in hits)
        one = md._match_from_hits(d, hits, 3)
        assert batched[i].model_dump() == one.model_dump(), d
    appmod.install_services(es, ms, md)
    try:
        with TestClient(appmod.app) as client:
            text = "霍乱，伤寒；副伤寒"
            plain = client.post("/query", json={"text": text, "top_k": 3})
            assert plain.status_code == 200 and plain.json()["candidates"]
            r = client.post("/query", json={"text": text, "top_k": 3, "radius": -1.0})
            assert r.status_code == 200 and r.json()["candidates"] == plain.json()["candidates"]
            r = client.post("/query", json={"text": text, "top_k": 3, "radius": 0.999})
            assert r.status_code == 200 and all(c["similarity_score"] is None or True for c in r.json()["candidates"])
            assert len(r.json()["candidates"]) <= len(plain.json()["candidates"])
            r = client.post("/query", json={"text": text, "top_k": 3, "radius": 5.0})
            assert r.status_code == 200 and r.json()["candidates"] == []
            assert client.post("/query", json={"text": text, "radius": 0.5, "range_filter": 0.5}).status_code == 400
            assert client.post("/query", json={"text": text, "radius": 0.7, "range_filter": 0.2}).status_code == 400
            assert client.post("/query", json={"text": text, "radius": 0.2, "group_by_field": "level"}).status_code == 400
            assert client.post("/query", json={"text": text, "radius": "high"}).status_code == 422
            assert client.post("/query", json={"text": text, "top_k": 3}).json() == plain.json()
    finally:
        appmod.install_services(None, None, None)
