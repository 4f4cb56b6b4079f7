"""Search by stored rows off the device: the contract's two statements in tests/byrows_oracle.py against
each other on random and adversarial lists, byrows_plan.hpp under the host sanitizers, the symbols, and MilvusService's
search_by_ids / similar_codes / knn_graph on their host side (argument checks, the unknown-code error, one library call per
batch) and the endpoint over a stub index."""
import os
import subprocess

import numpy as np
import pytest

import byrows_oracle as bo
from conftest import ROOT
from rag_project_icd10_amd import _native

CSRC = os.path.join(ROOT, "rag_project_icd10_amd", "csrc")


def test_plan_header_under_the_host_sanitizers(tmp_path):
    """tests/byrows_plan_check.cpp: the layout, id -> row at the edges, the gap and source slot at every k, whole lists (self first,
    in the middle, last, absent, padding, all tied) against erase-and-stable-sort - with ASan and UBSan"""
    exe = str(tmp_path / "byrows_plan_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(ROOT, "tests", "byrows_plan_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "byrows plan ok" in out.stdout


def test_symbols_and_abi():
    lib = _native.load_library()
    for name in ("icd_byrows_create", "icd_byrows_destroy", "icd_byrows_stats", "icd_index_search_by_rows"):
        assert hasattr(lib, name) and name in _native.EXPORTED_SYMBOLS
    assert lib.icd_abi_version() == _native.ABI_VERSION == 6
    header = open(os.path.join(ROOT, "include", "icd_search.h"), encoding="utf-8").read()
    assert "#define ICD_ABI_VERSION 6" in header
    assert "int icd_index_search_by_rows(icd_index *idx, icd_byrows *ws, icd_rowmask *const *masks, const int64_t *ids, int64_t nq, int32_t k," in header
    plan = open(os.path.join(CSRC, "byrows_plan.hpp"), encoding="utf-8").read()
    assert "hip/" not in plan and "__global__" not in plan                         # host only: no HIP header, no kernel
    kernel = open(os.path.join(CSRC, "byrows_kernel.hpp"), encoding="utf-8").read()
    body = kernel.split("#pragma once")[1]
    assert '#include "byrows_plan.hpp"' in kernel and "br_row_of(" in body and "br_gap(" in body and "br_source(" in body and "br_stable_rank(" in body
    assert "byrows_gather_kernel" in body and "byrows_drop_self_kernel" in body
    assert "atomic" not in body and "printf" not in body and "assert(" not in body
    # the checks that need no device: a destroyed / missing handle is ICD_ERR_STATE
    assert lib.icd_byrows_destroy(None) == -5 and lib.icd_byrows_stats(None, None, None) == -5
    assert lib.icd_index_search_by_rows(None, None, None, None, 0, 1, 0, 0, None, None, 0, 0, None, None, None, None, 0, None) == -5


# ---- the contract: two statements, one answer ---------------------------------------------------------------------------------
def ranking(rng, n, tied=False, id_base=0):
    """a full ranking of n rows, best first by (score desc, id asc), with runs of equal scores"""
    s = np.sort(rng.integers(-6, 7, n) / 8.0)[::-1].astype(np.float32) if not tied else np.full(n, 0.25, np.float32)
    ids = np.empty(n, np.int64)
    perm = rng.permutation(n)
    at = 0
    for v in sorted(set(s.tolist()), reverse=True):      # within a run of ties the ids ascend
        m = int((s == np.float32(v)).sum())
        ids[at:at + m] = np.sort(perm[at:at + m])
        at += m
    return s, ids + id_base


def both(scores, ids, levels, self_id, k, **kw):
    a = bo.without_self(scores, ids, levels, self_id, k, **kw)
    b = bo.drop_self(scores, ids, levels, self_id, k, **kw)
    for x, y in zip(a[0] + a[1], b[0] + b[1]):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), (self_id, k, kw, x, y)
    return a


def test_the_two_statements_agree_on_random_lists():
    rng = np.random.default_rng(5)
    for case in range(300):
        n = int(rng.integers(1, 40))
        id_base = int(rng.integers(0, 3)) * 1000
        s, ids = ranking(rng, n, tied=case % 7 == 0, id_base=id_base)
        levels = rng.integers(1, 4, n).astype(np.int32)
        k = int(rng.integers(1, n + 3))
        self_id = int(ids[rng.integers(0, n)])
        mask = None if case % 3 == 0 else rng.random(n) < 0.6
        kw = dict(mask=mask, id_base=id_base)
        if case % 4 == 1:
            kw["range_filter"] = float(s[min(n - 1, 2)])
        if case % 4 == 2 and float(s[-1]) < float(s[0]):
            kw["radius"] = float(s[-1])
        (raw, rid, lv), (adj, r_raw, r_ids, r_lv) = both(s, ids, levels, self_id, k, **kw)
        assert self_id not in rid.tolist() and len(rid) == k
        t = int((rid >= 0).sum())
        assert (rid[t:] == -1).all() and np.isneginf(raw[t:]).all() and (lv[t:] == 0).all()          # padding behind the hits
        assert sorted(r_ids[:t].tolist()) == sorted(rid[:t].tolist()) and (np.diff(adj[:t]) <= 0).all()
        # include_self: the masked search itself, and with self in its list the answer is that list without it
        full = both(s, ids, levels, self_id, k + 1, include_self=True, **kw)[0]
        if self_id in full[1].tolist():
            at = full[1].tolist().index(self_id)
            assert np.delete(full[1], at).tolist() == rid.tolist()
        else:
            assert full[1][:k].tolist() == rid.tolist()


def test_self_first_middle_last_absent_short_and_tied():
    levels = np.array([1, 2, 3, 1, 2, 3, 1, 2], np.int32)
    s = np.array([0.9, 0.8, 0.8, 0.8, 0.5, 0.5, 0.1, -0.2], np.float32)
    ids = np.array([4, 1, 3, 6, 0, 7, 2, 5], np.int64)
    first = both(s, ids, levels, 4, 3)[0]
    assert first[1].tolist() == [1, 3, 6] and first[0].tolist() == [np.float32(0.8)] * 3
    middle = both(s, ids, levels, 3, 3)[0]                                          # a tie with a smaller id comes first: self is rank 2
    assert middle[1].tolist() == [4, 1, 6]
    last = both(s, ids, levels, 5, 7)[0]
    assert last[1].tolist() == [4, 1, 3, 6, 0, 7, 2]
    absent = both(s, ids, levels, 4, 3, mask=np.array([1, 1, 1, 1, 0, 1, 1, 1], bool))[0]   # row 4 is outside its own mask
    assert absent[1].tolist() == [1, 3, 6]
    banded = both(s, ids, levels, 4, 3, range_filter=0.85)[0]                        # ... or outside its own band
    assert banded[1].tolist() == [1, 3, 6]
    short = both(s, ids, levels, 1, 10)[0]                                          # fewer rows than k: padding
    assert short[1].tolist() == [4, 3, 6, 0, 7, 2, 5, -1, -1, -1] and short[2].tolist()[-3:] == [0, 0, 0]
    tied = both(np.full(8, 0.0, np.float32), np.arange(8, dtype=np.int64), levels, 3, 4)
    assert tied[0][1].tolist() == [0, 1, 2, 4]                                      # all tied: id order, self cut out
    assert tied[1][2].tolist() == [0, 1, 2, 4]                                      # (adj = 0 for every level: the stable sort keeps it)
    one = both(np.array([1.0], np.float32), np.array([0], np.int64), levels, 0, 2)[0]
    assert one[1].tolist() == [-1, -1]                                              # n = 1: all padding
    # the reweighted form: the level weight reorders the k that stay (levels 1 / 2 / 3 weigh 1.2 / 1.0 / 0.8)
    rew = both(s, ids, levels, 4, 3)[1]
    assert rew[2].tolist() == [3, 6, 1] and rew[0].tolist() == [float(np.float64(np.float32(0.8)) * w) for w in (1.2, 1.2, 1.0)]
    # the masked search's REWEIGHTED list at k + 1 gives the same answer: self present, and absent (the raw-last entry goes)
    for self_id, kw in ((4, {}), (3, {}), (4, dict(mask=np.array([1, 1, 1, 1, 0, 1, 1, 1], bool))), (1, dict(range_filter=0.6))):
        for k in (1, 3, 5, 9):
            want = bo.without_self(s, ids, levels, self_id, k, **kw)[1]
            wide = bo.without_self(s, ids, levels, self_id, k + 1, include_self=True, **kw)[1]
            got = bo.drop_reweighted_list(*wide, self_id)
            for x, y in zip(got, want):
                assert x.tobytes() == y.tobytes(), (self_id, kw, k)


# ---- the service on its host side ---------------------------------------------------------------------------------------------
class StubMask:
    def __init__(self, rows, transient=False):
        self.rows, self.closed, self.transient = len(rows), False, transient

    def stats(self):
        return {"rows": self.rows, "bytes": 0}

    def close(self):
        self.closed = True


class StubWorkspace:
    def __init__(self, max_nq):
        self.max_nq, self.closed = max_nq, False

    def close(self):
        self.closed = True


class StubIndex:
    """IcdIndex as search_by_ids sees it: every call is noted; the hits of id i are rows i + 1, i + 2, ... (mod n)"""

    def __init__(self, n, dim, max_nq=8, max_k=64):
        self.n, self.dim, self.max_nq, self.max_k, self.device, self.closed = n, dim, max_nq, max_k, 0, False
        self.calls, self.made, self.handles = [], [], []

    def rowmask(self, rows):
        self.made.append(len(rows))
        return StubMask(rows)

    def byrows(self, max_nq=None):
        self.handles.append(StubWorkspace(max_nq))
        return self.handles[-1]

    def search_by_rows(self, ids, k, *, workspace, masks=None, radius=None, range_filter=None, include_self=False, reweighted=True, on_device=False):
        ids = np.asarray(ids, np.int64)
        assert ids.ndim == 1 and not workspace.closed and reweighted   # (a longer batch runs in chunks inside the wrapper)
        assert masks is None or (len(masks) == len(ids) and all(m is None or not m.closed for m in masks))
        self.calls.append(dict(ids=ids.tolist(), k=k, masks=masks, radius=radius, range_filter=range_filter, include_self=include_self))
        out = (ids[:, None] + np.arange(0 if include_self else 1, k + (0 if include_self else 1))[None, :]) % self.n
        out[:, self.n - (0 if include_self else 1):] = -1
        raw = np.where(out >= 0, 0.5 - 0.01 * np.arange(k)[None, :], -np.inf).astype(np.float32)
        return raw.astype(np.float64), raw, out.astype(np.int64), np.where(out >= 0, 2, 0).astype(np.int32)

    def close(self):
        self.closed = True


RECORDS = [{"code": c, "preferred_zh": t, "level": lv, "parent_code": p, "has_complication": False, "main_code": None, "secondary_code": None,
            "category_path": ""}
           for c, t, lv, p in [("A00", "霍乱", 1, ""), ("A00.0", "霍乱，由于O1群霍乱弧菌", 2, "A00"), ("A00.1", "埃尔托霍乱", 2, "A00"),
                               ("A01", "伤寒和副伤寒", 1, ""), ("A01.0", "伤寒", 2, "A01"), ("A01.1", "副伤寒甲", 2, "A01")]]
DIM = 64


@pytest.fixture()
def svc(tmp_path, monkeypatch):
    monkeypatch.setenv("MILVUS_DB_PATH", str(tmp_path / "db"))
    monkeypatch.setenv("MILVUS_COLLECTION_NAME", "byrows")
    from rag_project_icd10_amd.services.milvus_service import MilvusService

    class Emb:                      # (the store takes its dimension from the encoder)
        def encode_query(self, t):
            return np.ones(DIM, np.float32) / 8

    class Small(MilvusService):
        FILTER_ON_DEVICE = False    # the host route: filter_rows -> index.rowmask
        TEXT_MATCH_ON_DEVICE = False

    s = Small(Emb())
    yield s
    s.disconnect()


def load(svc, **kw):
    rng = np.random.default_rng(0)
    assert svc.insert_records(RECORDS, [rng.standard_normal(DIM).astype(np.float32) for _ in RECORDS]) is True
    svc._index = StubIndex(len(RECORDS), DIM, **kw)
    svc._index_rows, svc._index_gen = svc.client.count, svc.client.generation
    return svc._index


def test_empty_collection(svc):
    assert svc.search_by_ids([0, 1], 3) == [[], []] and svc.search_by_ids(0, 3, filter="level == 2") == [[]]
    ids, scores = svc.knn_graph(4)
    assert ids.shape == scores.shape == (0, 4) and ids.dtype == np.int64 and scores.dtype == np.float64
    with pytest.raises(KeyError):
        svc.similar_codes("A00")                 # no collection holds no code
    for bad in (lambda: svc.search_by_ids([0], 0), lambda: svc.search_by_ids([0], 3, filter="level =="), lambda: svc.knn_graph(128),
                lambda: svc.similar_codes("A00", 0)):
        with pytest.raises(ValueError):          # a bad argument raises on an empty collection too
            bad()


def test_argument_checks(svc):
    index = load(svc)
    bad = [
        lambda: svc.search_by_ids([0], 0), lambda: svc.search_by_ids([0], -1), lambda: svc.search_by_ids([0], 128), lambda: svc.search_by_ids([0], 2.5),
        lambda: svc.search_by_ids([0], True), lambda: svc.search_by_ids([0], "3"), lambda: svc.search_by_ids([0], 129, include_self=True),
        lambda: svc.search_by_ids([0], 64),                                         # 64 + 1 is above the store's max k (64)
        lambda: svc.search_by_ids([0], 65, include_self=True),
        lambda: svc.search_by_ids([6], 3), lambda: svc.search_by_ids([0, -1], 3), lambda: svc.search_by_ids([0, 10 ** 12], 3),   # no rows of the collection
        lambda: svc.search_by_ids("0", 3), lambda: svc.search_by_ids([0.5], 3), lambda: svc.search_by_ids([True], 3), lambda: svc.search_by_ids([[0, 1]], 3),
        lambda: svc.search_by_ids(None, 3),
        lambda: svc.search_by_ids([0], 3, filter="level =="), lambda: svc.search_by_ids([0], 3, filter="nope == 1"),
        lambda: svc.search_by_ids([0, 1], 3, filter=["level == 2"]), lambda: svc.search_by_ids([0, 1], 3, filter=["level == 2", "level =="]),
        lambda: svc.search_by_ids([0], 3, radius=0.5, range_filter=0.1), lambda: svc.search_by_ids([0], 3, radius=float("nan")),
        lambda: svc.search_by_ids([0], 3, radius="x"),
        lambda: svc.similar_codes("A00", 0), lambda: svc.similar_codes("A00", 128), lambda: svc.similar_codes("", 3), lambda: svc.similar_codes(7, 3),
        lambda: svc.similar_codes('A"00', 3), lambda: svc.similar_codes("A00", 3, filter="level =="), lambda: svc.similar_codes("A00", 3, filter=["level == 2"]),
        lambda: svc.knn_graph(0), lambda: svc.knn_graph(128), lambda: svc.knn_graph(64), lambda: svc.knn_graph(3, filter="level =="),
        lambda: svc.knn_graph(3, filter=["level == 2"]),
    ]
    for i, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
            pytest.fail(f"case {i} did not raise")
    for code in ("Z99", "a00", "A00 "):          # an unknown code is a KeyError, not an empty list
        with pytest.raises(KeyError):
            svc.similar_codes(code, 3)
    assert index.calls == [] and index.made == [] and index.handles == []      # every check came before the index was asked


def test_the_hits_and_one_call_per_batch(svc):
    index = load(svc)
    adj, raw, ids, levels = svc.search_by_ids([0, 4, 4], 3)
    assert adj.shape == raw.shape == ids.shape == levels.shape == (3, 3) and ids.tolist() == [[1, 2, 3], [5, 0, 1], [5, 0, 1]]
    assert len(index.calls) == 1 and index.calls[0]["ids"] == [0, 4, 4] and index.calls[0]["masks"] is None and len(index.handles) == 1
    hits = svc.search_by_ids(4, 2, as_dicts=True)                                   # one id, not a list
    assert [h["code"] for h in hits[0]] == ["A01.1", "A00"] and len(index.handles) == 1   # the workspace is kept
    assert hits[0][0] == svc._hits_to_dicts(np.float64([np.float32(0.5)]), np.float32([0.5]), np.int64([5]))[0]   # `search`'s dict
    assert len(svc.search_by_ids([0], 10, as_dicts=True)[0]) == len(RECORDS) - 1     # padding is dropped
    svc.search_by_ids([0], 64, include_self=True)
    assert index.calls[-1]["include_self"] is True and index.calls[-1]["k"] == 64
    svc.search_by_ids([1], 3, radius=0.1, range_filter=0.9)
    assert index.calls[-1]["radius"] == float(np.float32(0.1)) and index.calls[-1]["range_filter"] == float(np.float32(0.9))
    # similar_codes: the code's row is the id
    sim = svc.similar_codes("A01", 2)
    assert index.calls[-1]["ids"] == [3] and [h["code"] for h in sim] == ["A01.0", "A01.1"]
    # per-id filters: one masks call, equal expressions share a mask, no filter is a NULL entry
    before = len(index.calls)
    filters = ["level == 2", None, 'code like "A01%"', "level == 2", "level > 5"]
    lists = svc.search_by_ids([0, 1, 2, 3, 4], 3, filter=filters, as_dicts=True)
    assert len(index.calls) == before + 1 and len(lists) == 5
    masks = index.calls[-1]["masks"]
    assert masks[1] is None and masks[0] is masks[3] and index.made == [4, 3, 0]
    svc.similar_codes("A00", 2, filter="level == 2")
    assert index.calls[-1]["masks"][0] is masks[0]                                  # the cached mask of the same expression
    # a batch longer than the workspace: a larger one is made, up to the index's max_nq
    svc.search_by_ids(list(range(6)) * 12, 2)
    assert len(index.handles) == 2 and index.handles[-1].max_nq == index.max_nq


def test_endpoint_over_the_stub(svc):
    fastapi = pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient
    from rag_project_icd10_amd.api import app as api
    index = load(svc)
    saved = (api.embedding_service, api.milvus_service, api.multi_diagnosis_service)
    api.install_services(None, svc, multi=object())
    try:
        client = TestClient(api.app)
        r = client.get("/codes/A01/similar", params={"top_k": 2})
        assert r.status_code == 200, r.text
        body = r.json()
        want = svc.similar_codes("A01", 2)
        assert body["code"] == "A01" and [c["code"] for c in body["candidates"]] == [h["code"] for h in want] == ["A01.0", "A01.1"]
        assert [c["score"] for c in body["candidates"]] == [h["score"] for h in want]
        assert [c["original_score"] for c in body["candidates"]] == [h["original_score"] for h in want]
        assert client.get("/codes/Z99/similar").status_code == 404
        assert client.get("/codes/A01/similar", params={"top_k": 0}).status_code == 400
        assert client.get("/codes/A01/similar", params={"filter": "level =="}).status_code == 400
        r = client.get("/codes/A01/similar", params={"top_k": 3, "filter": "level == 2"})
        assert r.status_code == 200 and index.calls[-1]["masks"][0] is not None
        assert client.get("/codes/A01").status_code in (200, 500)                   # (the record route still resolves: the new path did not shadow it)
    finally:
        api.embedding_service, api.milvus_service, api.multi_diagnosis_service = saved
    assert fastapi is not None
