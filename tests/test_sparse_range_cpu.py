"""The sparse range search's host side, no device: the oracle against sparse_oracle.search and against its
own pages, the Python argument rules, the library's refusals that come before any device call, the refusal that stays (bounds on a
sparse AnnSearchRequest inside hybrid_search)."""
import types

import numpy as np
import pytest

import sparse_oracle as so
import sparse_range_oracle as sro
from rag_project_icd10_amd import _native
from rag_project_icd10_amd.services import range_search
from rag_project_icd10_amd.services.hybrid_search import AnnSearchRequest
from rag_project_icd10_amd.services.milvus_service import MilvusService


def _world(seed=5, n=400, vocab=12):
    """rows with ties (few distinct values, either sign) and queries of 0 .. 5 terms; every product a normal float"""
    rng = np.random.default_rng(seed)
    row_off, terms, vals = [0], [], []
    for _ in range(n):
        t = np.flatnonzero(rng.random(vocab) < 0.3)
        terms += t.tolist()
        vals += rng.choice([0.5, 1.0, -2.0, 3.0], len(t)).tolist()
        row_off.append(len(terms))
    rows = (np.array(row_off, np.int64), np.array(terms, np.uint32), np.array(vals, np.float32))
    q_off, q_terms, q_vals = [0], [], []
    for q in range(9):
        t = np.sort(rng.choice(vocab, q % 6, replace=False))
        q_terms += t.tolist()
        q_vals += rng.choice([1.0, -1.0, 0.25], len(t)).tolist()
        q_off.append(len(q_terms))
    q = (np.array(q_off, np.int64), np.array(q_terms, np.uint32), np.array(q_vals, np.float32))
    levels = rng.integers(1, 4, n).astype(np.int32)
    return rows, q, levels, vocab


def test_no_bounds_equals_the_sparse_oracle():
    rows, q, levels, vocab = _world()
    scored = sro.score_queries(*rows, vocab, *q)
    masks = [None if i % 2 else (np.arange(400) % 3 != 0) for i in range(9)]
    for k in (1, 10, 128):
        for rw in (False, True):
            want = so.search(*rows, vocab, *q, k, levels=levels, id_base=70, masks=masks, reweighted=rw)
            got = sro.search(scored, k, levels=levels, id_base=70, masks=masks, reweighted=rw)
            assert all(g.dtype == w.dtype and g.tobytes() == w.tobytes() for g, w in zip(got, want)), (k, rw)
    assert (sro.search(scored, 5)[1][0] == -1).all()   # the query without terms: padding


def test_order_f32_orders_as_make_key_does():
    x = np.array([-np.inf, -3.0, -1e-30, -0.0, 0.0, 1e-30, 0.5, np.inf], np.float32)
    o = sro.order_f32(x).astype(np.int64)
    assert (np.diff(o) > 0).all()
    assert o[3] == 0x7FFFFFFF and o[4] == 0x80000000


def test_pages_by_cursor_concatenate_to_the_full_ranking():
    rows, q, levels, vocab = _world(seed=9)
    scored = sro.score_queries(*rows, vocab, *q)
    for qi in (1, 3, 5):
        acc, hit = scored[qi]
        for kw in ({}, {"radius": 0.0}, {"range_filter": 1.0}, {"radius": -2.0, "range_filter": 3.0}):
            full = sro.rankings([scored[qi]], id_base=7, **kw)[0][1].tolist()
            assert len(full) > 20 or kw
            for batch in (1, 16, 128):
                pg = sro.pages(acc, hit, batch, id_base=7, **kw)
                assert [i for p in pg for i in p] == full and all(len(p) == batch for p in pg[:-1])
            cut = sro.pages(acc, hit, 16, id_base=7, limit=20, **kw)
            assert [i for p in cut for i in p] == full[:20]
    # the band is applied to the hits: a floor of -inf admits no row without a shared term
    acc, hit = scored[1]
    assert not hit.all() and len(sro.band_rows(acc, hit, radius=-np.inf)) == int(hit.sum())
    # radius excludes an equal score, range_filter includes it
    s = float(acc[sro.band_rows(acc, hit)[3]])
    assert (acc[sro.band_rows(acc, hit, radius=s)] > s).all() and acc[sro.band_rows(acc, hit, range_filter=s)][0] == s


def test_python_argument_rules():
    ms = MilvusService.__new__(MilvusService)
    ms.client = None
    ms.collection_name = "none"
    ms._sparse = None
    off, t, v = np.array([0, 1], np.int64), np.array([0], np.uint32), np.array([1.0], np.float32)
    bad = ({"radius": float("nan")}, {"range_filter": float("nan")}, {"radius": 0.5, "range_filter": 0.5}, {"radius": 2.0, "range_filter": 1.0},
           {"offset": -1}, {"offset": 16384 - 4}, {"radius": "high"}, {"radius": 0.1, "group_by_field": "level"},
           {"range_filter": 0.1, "group_by_field": "level"}, {"offset": 2, "group_by_field": "level"})
    for kw in bad:
        with pytest.raises(ValueError):
            ms.search_text("肺炎", 5, **kw)
        with pytest.raises(ValueError):
            ms.search_sparse_batch(off, t, v, 5, **kw)
    with pytest.raises(ValueError):
        ms.search_text("肺炎", 5, search_params={"params": {"radius": 2, "range_filter": 1}})
    for kw in ({"radius": float("nan")}, {"radius": 1.0, "range_filter": 1.0}, {"batch_size": 0}, {"batch_size": 129}, {"limit": -2},
               {"filter": "level >>> 3"}, {"filter": ["level >= 2"]}):
        with pytest.raises(ValueError):
            ms.search_text_iterator("肺炎", **kw)
    # per-query arrays: every query's pair is checked
    off2 = np.array([0, 1, 1], np.int64)
    for kw in ({"radius": np.array([0.1, np.nan], np.float32)}, {"radius": np.array([0.1, 0.9]), "range_filter": 0.5},
               {"radius": np.array([0.1, 0.2, 0.3])}, {"range_filter": np.array([0.1])[:0]}):
        with pytest.raises(ValueError):
            ms.search_sparse_batch(off2, t, v, 5, **kw)
    r, f = range_search.check_bounds_per_query(np.array([0.1, 0.2]), 0.5, 2)
    assert r.dtype == np.float32 and r.tolist() == [np.float32(0.1), np.float32(0.2)] and f == 0.5
    assert range_search.check_bounds_per_query(None, 3, 2) == (None, 3.0)
    assert range_search.check_offset(16384 - 5, 5) == 16384 - 5
    # IcdIndex.search_sparse: the rules that come before the library is asked
    this = types.SimpleNamespace(closed=False)
    sp, grouping = types.SimpleNamespace(closed=False), types.SimpleNamespace(closed=False)
    for kw in ({"radius": 0.5}, {"range_filter": 0.5}, {"after": (1.0, 3)}):
        with pytest.raises(ValueError, match="grouping"):
            _native.IcdIndex.search_sparse(this, sp, off, t, v, 5, grouping=grouping, group_size=2, **kw)
    for after in ((1.0, None), (None, 3)):
        with pytest.raises(ValueError, match="both or neither"):
            _native.IcdIndex.search_sparse(this, sp, off, t, v, 5, after=after)
    # the adapter's surface
    band = range_search.SparseBandIndex(types.SimpleNamespace(closed=False, max_k=100), types.SimpleNamespace(closed=False, max_k=128, max_nq=4), None)
    assert band.max_k == 100 and not band.closed
    band.sparse.closed = True
    assert band.closed
    it = range_search.SearchIterator(None, None, 10, -1, None, None, None, lambda: 0)
    assert it.next() == []


def test_library_refusals_before_any_device_call():
    lib = _native.load_library()
    assert "icd_sparse_search_range" in _native.EXPORTED_SYMBOLS and hasattr(lib, "icd_sparse_search_range")
    # handles that are not: ICD_ERR_STATE
    assert lib.icd_sparse_search_range(None, None, None, None, None, 1, 1, 0, None, None, None, None, None, 0, 0, None, None, None, None, 0, None) == -5
    nan = np.array([np.nan], np.float32)
    assert lib.icd_sparse_search_range(None, None, None, None, None, 1, 1, 0, None, nan.ctypes.data, None, None, None, 0, 0, None, None, None, None, 0, None) == -5
    assert b"invalid handle" in lib.icd_last_error()


def test_a_sparse_request_with_a_radius_is_still_refused():
    with pytest.raises(ValueError):
        AnnSearchRequest("肺炎", 5, param={"params": {"radius": 0.1}}, anns_field="sparse")
    with pytest.raises(ValueError):
        AnnSearchRequest("肺炎", 5, param={"params": {"range_filter": 0.1}}, anns_field="sparse")
