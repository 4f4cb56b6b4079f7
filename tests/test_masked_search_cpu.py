"""Masked search, the parts that need no GPU: the oracle helper against brute force, the host bitset packer against
numpy.packbits, the argument checks of MilvusService and /query, the exported symbols."""
import ctypes

import numpy as np
import pytest

from mask_oracle import brute_force_topk, masked_batch, masked_pages, restrict
from range_oracle import band_batch

from rag_project_icd10_amd import _native


def _tiny(n=500, dim=16, nq=12, seed=5):
    """integer-valued rows and queries: every inner product is exact in fp32 AND fp64, whatever the summation order, so a plain
    numpy ranking is a yardstick without rounding questions; plenty of exact ties"""
    rng = np.random.default_rng(seed)
    corpus = rng.integers(-4, 5, (n, dim)).astype(np.float32)
    q = rng.integers(-4, 5, (nq, dim)).astype(np.float32)
    levels = rng.integers(1, 4, n).astype(np.int32)
    sc = (corpus.astype(np.float64) @ q.astype(np.float64).T).T.astype(np.float32)
    order = np.stack([np.lexsort((np.arange(n), -sc[i])) for i in range(nq)])
    return corpus, q, levels, np.take_along_axis(sc, order, 1), order.astype(np.int64)


def test_mask_oracle_against_brute_force():
    corpus, q, levels, s_all, i_all = _tiny()
    n, nq = corpus.shape[0], q.shape[0]
    rows = np.arange(n)
    sels = [None, rows % 7 == 3, rows < 40, np.zeros(n, bool), rows >= 490, np.nonzero(rows % 2 == 1)[0]] * 2
    for k in (1, 10, 64):
        (raw, ids, lv), (adj, raw2, ids2, lv2) = masked_batch(s_all, i_all, levels, sels, k)
        for qi in range(nq):
            sel_rows = rows if sels[qi] is None else (np.nonzero(sels[qi])[0] if np.asarray(sels[qi]).dtype == bool else sels[qi])
            want = brute_force_topk(corpus, q[qi], sel_rows, k)
            m = len(want)
            assert m == min(k, len(sel_rows))
            assert np.array_equal(ids[qi, :m], want) and (ids[qi, m:] == -1).all() and np.isneginf(raw[qi, m:]).all()
            assert np.array_equal(raw[qi, :m], (corpus[want].astype(np.float64) @ q[qi].astype(np.float64)).astype(np.float32))
            assert np.array_equal(lv[qi, :m], levels[want]) and (lv[qi, m:] == 0).all()
            # reweighted: the same hits, adjusted scores descending, padding behind
            assert sorted(ids2[qi, :m].tolist()) == sorted(want.tolist()) and (np.diff(adj[qi, :m]) <= 0).all()
    # no mask anywhere = the band oracle itself; bounds apply to the RESTRICTED ranking
    a = masked_batch(s_all, i_all, levels, [None] * nq, 10, radius=1.0)
    b = band_batch(s_all, i_all, levels, 10, radius=1.0)
    assert all(np.array_equal(x, y) for x, y in zip(a[0] + a[1], b[0] + b[1]))
    sel = rows % 3 == 0
    s_r, i_r = restrict(s_all[0], i_all[0], sel)
    assert sel[i_r].all() and len(i_r) == int(sel.sum()) and (np.diff(s_r) <= 0).all()
    (raw, ids, _lv), _ = masked_batch(s_all[:1], i_all[:1], levels, [sel], 5, after=(s_r[4:5], i_r[4:5]))
    assert np.array_equal(ids[0], i_r[5:10])
    # a cursor on a masked-OUT row cuts the restricted ranking where that row would stand
    out_pos = int(np.nonzero(~sel[i_all[0]])[0][6])
    (raw, ids, _lv), _ = masked_batch(s_all[:1], i_all[:1], levels, [sel], 5, after=(s_all[0, out_pos:out_pos + 1], i_all[0, out_pos:out_pos + 1]))
    behind = [i for i in i_all[0, out_pos + 1:] if sel[i]][:5]
    assert ids[0].tolist() == behind
    pages = masked_pages(s_all[0], i_all[0], sel, 7)
    assert [i for p in pages for i in p] == i_r.tolist() and all(len(p) == 7 for p in pages[:-1])


@pytest.mark.parametrize("n", [1, 31, 32, 33, 127, 128, 129, 500, 4099, 12000])
def test_host_packer_against_numpy_packbits(n):
    rng = np.random.default_rng(n)
    for sel in (rng.random(n) < 0.5, np.zeros(n, bool), np.ones(n, bool), np.arange(n) == n - 1, np.arange(n) % 128 == 37 % n):
        words = _native.pack_rowmask(np.nonzero(sel)[0], n)
        assert words.dtype == np.uint32 and len(words) == _native.rowmask_words(n) == (n + 127) // 128 * 4
        padded = np.zeros(len(words) * 32, bool)
        padded[:n] = sel
        want = np.packbits(padded, bitorder="little").view("<u4")
        assert np.array_equal(words, want)
        assert not np.unpackbits(words.view(np.uint8), bitorder="little")[n:].any()   # zero padding up to the tile boundary
    lib = _native.load_library()
    out = np.full(_native.rowmask_words(n) + 3, 0xFFFFFFFF, np.uint32)   # a longer buffer is zero-filled to its end
    r = np.array([0], np.int64)
    assert lib.icd_rowmask_pack(r.ctypes.data, 1, n, out.ctypes.data, len(out)) == 0 and out[0] == 1 and not out[1:].any()
    for bad in ([0, 0], [1, 0], [-1], [n]):
        with pytest.raises(ValueError):
            _native.pack_rowmask(np.array(bad), n)
    assert lib.icd_rowmask_pack(r.ctypes.data, 1, n, out.ctypes.data, _native.rowmask_words(n) - 1) == -1   # buffer too short


def test_library_exports_the_rowmask_symbols_and_keeps_the_abi_version():
    lib = _native.load_library()
    for name in ("icd_rowmask_create", "icd_rowmask_destroy", "icd_rowmask_stats", "icd_index_search_masked", "icd_rowmask_pack"):
        assert hasattr(lib, name) and name in _native.EXPORTED_SYMBOLS, name
    assert lib.icd_abi_version() == 6 == _native.ABI_VERSION
    # the checks that need no device answer with a status before any HIP call
    out = ctypes.c_void_p()
    assert lib.icd_rowmask_create(None, None, 0, 0, ctypes.byref(out)) == -5 and not out.value      # ICD_ERR_STATE: no index
    assert lib.icd_rowmask_destroy(None) == -5 and lib.icd_rowmask_stats(None, None, None) == -5
    q = np.zeros((1, 64), np.float32)
    masks = (ctypes.c_void_p * 1)(None)
    assert lib.icd_index_search_masked(None, masks, q.ctypes.data, 1, 5, 0, None, None, None, None, 0, 0, None, None, None, None, 0, None) == -5


def test_milvus_service_filter_argument_checks_need_no_device(tmp_path, monkeypatch):
    monkeypatch.setenv("MILVUS_DB_PATH", str(tmp_path / "db"))
    monkeypatch.setenv("MILVUS_COLLECTION_NAME", "m")
    from rag_project_icd10_amd.services.milvus_service import MilvusService

    class Emb:
        def encode_query(self, t):
            return np.ones(64, np.float32) / 8

    svc = MilvusService(Emb())
    recs = [{"code": c, "preferred_zh": c, "level": lv, "main_code": None, "secondary_code": None} for c, lv in (("A00", 1), ("A00.1", 2), ("B01", 2))]
    assert svc.insert_records(recs, [np.ones(64, np.float32) * (i + 1) for i in range(3)]) is True

    def no_device(*a, **k):
        raise AssertionError("an argument error must be raised before the index is loaded")
    monkeypatch.setattr(svc, "_ready_index", no_device)
    vecs = np.ones((2, 64), np.float32)
    bad_calls = [
        dict(filter=["level >= 2"]),                                      # wrong list length
        dict(filter=["level >= 2", "level >= 2", None]),
        dict(filter=["level >= 2", "level >"]),                           # a bad expression inside a list
        dict(filter=("level >= 2", None), group_by_field="level"),        # a list next to grouping
        dict(filter="level >= 2", filter_mode="mask", group_by_field="level"),
        dict(filter="level >= 2", filter_mode="bitmap"),                  # bad filter_mode
        dict(filter_mode="MASK"),
        dict(filter="level >", filter_mode="mask"),
    ]
    for kw in bad_calls:
        with pytest.raises(ValueError):
            svc.search_batch(vecs, 2, **kw)
    # the default path still takes whatever array-like it took (a nested list has no .shape): it gets as far as the index
    with pytest.raises(AssertionError, match="before the index is loaded"):
        svc.search_batch(vecs.tolist(), 2)
    with pytest.raises(AssertionError, match="before the index is loaded"):
        svc.search_batch(vecs.tolist(), 2, filter="level >= 2")
    with pytest.raises(ValueError):
        svc.search_batch(vecs.tolist(), 2, filter=["level >= 2"])      # (a list of filters counts a nested list's queries too)
    for kw in (dict(filter_mode="bitmap"), dict(filter="level >= 2", filter_mode=None), dict(filter=["level >= 2"]),
               dict(filter="level >= 2", filter_mode="mask", group_by_field="level")):
        with pytest.raises(ValueError):
            svc.search(vecs[0], 2, **kw)
    for kw in (dict(filter_mode="bitmap"), dict(filter="level >", filter_mode="mask"), dict(filter=["level >= 2"])):
        with pytest.raises(ValueError):
            svc.search_iterator(vecs[0], batch_size=2, **kw)
    assert svc.filter_masks() == [] and svc.filter_views() == []
    from rag_project_icd10_amd.services.multi_diagnosis_service import _search_options
    assert _search_options("level >= 2", None, 1) == {"filter": "level >= 2"}                       # the default mode adds nothing
    assert _search_options(["a", None], None, 1, filter_mode="mask") == {"filter": ["a", None], "filter_mode": "mask"}


def test_query_endpoint_rejects_a_bad_filter_mode():
    from fastapi.testclient import TestClient
    from rag_project_icd10_amd.api import app as appmod

    class Emb:
        def encode_query_batch(self, qs, **kw):
            return np.zeros((len(qs), 2), np.float32)

        def get_model_info(self):
            return {"loaded": True, "model_name": "stub"}

    class Mil:
        def __init__(self):
            self.seen = []

        def search_batch(self, v, k, as_dicts=False, **kw):
            self.seen.append(kw)
            return [[{"code": "I21.9", "title": "t", "score": 0.9, "original_score": 0.9, "metadata": {"level": 2}}][:k] for _ in range(len(v))]

        def filter_masks(self):
            return [{"expression": "level >= 2", "rows": 2, "generation": 1, "bytes": 32}]

        def get_collection_stats(self):
            return {"num_entities": 3}

        def test_connection(self):
            return {"connected": True}

        def disconnect(self):
            return {}

    mil = Mil()
    appmod.install_services(Emb(), mil)
    try:
        with TestClient(appmod.app) as client:
            r = client.post("/query", json={"text": "高血压", "top_k": 1, "filter": "level >= 2", "filter_mode": "bitmap"})
            assert r.status_code == 400 and "filter_mode" in r.json()["detail"]
            assert client.post("/query", json={"text": "高血压", "top_k": 1, "filter_mode": ""}).status_code == 400
            r = client.post("/query", json={"text": "高血压", "top_k": 1, "filter": "level >= 2", "filter_mode": "mask", "group_by_field": "level"})
            assert r.status_code == 400
            assert mil.seen == []
            assert client.post("/query", json={"text": "高血压", "top_k": 1, "filter": "level >= 2", "filter_mode": "mask"}).status_code == 200
            assert mil.seen[-1] == {"filter": "level >= 2", "filter_mode": "mask"}
            assert client.post("/query", json={"text": "高血压", "top_k": 1, "filter": "level >= 2"}).status_code == 200
            assert mil.seen[-1] == {"filter": "level >= 2"}                                          # the default: today's call
            assert client.get("/stats").json()["filter_masks"] == mil.filter_masks()
    finally:
        appmod.install_services(None, None, None)


@pytest.mark.parametrize("id_base", [1000, 2**32 + 12345])
def test_a_ranking_shifted_by_id_base_gives_the_same_outputs_with_the_ids_shifted(id_base):
    corpus, q, levels, s_all, i_all = _tiny()
    n, nq = corpus.shape[0], q.shape[0]
    rows = np.arange(n)
    sels = [None, rows % 7 == 3, rows < 40, np.zeros(n, bool), rows >= 490, np.nonzero(rows % 2 == 1)[0]] * 2   # masks stay over ROWS
    shift = lambda a: np.where(a >= 0, a + id_base, a)
    cur = (s_all[:, 9].copy(), i_all[:, 9].copy())
    for case in (dict(), dict(radius=s_all[:, 60].copy()), dict(range_filter=s_all[:, 20].copy(), after=cur), dict(offset=2)):
        for k in (1, 10, 64):
            want_raw, want_adj = masked_batch(s_all, i_all, levels, sels, k, **case)
            moved = dict(case)
            if "after" in case:
                moved["after"] = (cur[0], cur[1] + id_base)
            got_raw, got_adj = masked_batch(s_all, i_all + id_base, levels, sels, k, id_base=id_base, **moved)
            for j, (g, w) in enumerate(zip(got_raw + got_adj, want_raw + want_adj)):
                assert g.dtype == w.dtype and g.tobytes() == (shift(w) if w.dtype == np.int64 else w).tobytes(), (sorted(case), k, j)
    s_r, i_r = restrict(s_all[0], i_all[0] + id_base, sels[1], id_base)
    assert np.array_equal(i_r - id_base, restrict(s_all[0], i_all[0], sels[1])[1]) and np.array_equal(s_r, restrict(s_all[0], i_all[0], sels[1])[0])
