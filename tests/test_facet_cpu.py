"""Facet counts without a GPU: the host-only plan header under the host sanitizers, the exported symbol and
the ABI version, the numpy oracle against a plain loop, MilvusService.facet / facet_batch on their host side - argument checks, the
empty collection, ordering, min_count and limit, the release of a search's own masks - over a stub index that answers group_counts
from the oracle, and the API route over a stub service."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import facet_oracle as fo
from conftest import ROOT
from rag_project_icd10_amd import _native

CSRC = os.path.join(ROOT, "rag_project_icd10_amd", "csrc")


def test_plan_header_under_the_host_sanitizers(tmp_path):
    """tests/facet_count_plan_check.cpp: the host-only header that holds the segment, form and pass arithmetic, in a program of
    its own, with ASan and UBSan"""
    exe = str(tmp_path / "facet_count_plan_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(ROOT, "tests", "facet_count_plan_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "facet count plan ok" in out.stdout


def test_symbol_abi_and_the_checks_that_need_no_device():
    lib = _native.load_library()
    assert hasattr(lib, "icd_rowmask_group_counts") and "icd_rowmask_group_counts" in _native.EXPORTED_SYMBOLS
    assert lib.icd_abi_version() == _native.ABI_VERSION == 6
    header = open(os.path.join(ROOT, "include", "icd_search.h"), encoding="utf-8").read()
    assert "int icd_rowmask_group_counts(icd_index *idx, icd_grouping *grouping, icd_rowmask *const *masks, int64_t nq," in header
    assert "#define ICD_ABI_VERSION 6" in header
    plan = open(os.path.join(CSRC, "facet_count_plan.hpp"), encoding="utf-8").read()
    assert "hip/" not in plan and "__global__" not in plan                         # host only: no HIP header, no kernel
    assert f"#define ICD_FC_LDS_GROUPS {_native.FACET_LDS_GROUPS}" in plan and _native.FACET_LDS_GROUPS == 8192
    kernel = open(os.path.join(CSRC, "facet_count_kernel.hpp"), encoding="utf-8").read()
    assert '#include "facet_count_plan.hpp"' in kernel and "ms_lane_bits(" in kernel and "__device__ __forceinline__ unsigned long long ms_lane_bits" not in kernel
    assert "float" not in kernel.split("#pragma once")[1]                          # no float is added anywhere
    counts = np.full((2, 3), -7, np.int32)
    table = (ctypes.c_void_p * 2)()
    call = lambda idx, grp, nq, tab=table, out=counts: lib.icd_rowmask_group_counts(   # noqa: E731
        idx, grp, None if tab is None else ctypes.cast(tab, ctypes.c_void_p), nq, None if out is None else out.ctypes.data, 0, None)
    assert call(None, None, -1) == -1 and b"nq=-1" in lib.icd_last_error()          # ICD_ERR_INVALID before the handles are looked at
    assert call(None, None, 2, None) == -1 and call(None, None, 2, table, None) == -1
    assert call(None, None, 2) == -5 and call(None, None, 0) == -5                  # ICD_ERR_STATE: no index
    assert (counts == -7).all()


def test_oracle_against_a_loop():
    rng = np.random.default_rng(5)
    for n in (1, 33, 200):
        for ids in (np.zeros(n, np.int64), np.arange(n) % 2, np.arange(n), np.array([5, 1000, 7])[rng.integers(0, 3, n)]):
            group_ids, dense_of = fo.dense(ids)
            assert group_ids.tolist() == sorted(set(ids.tolist())) and (group_ids[dense_of] == ids).all()
            for density in (0.0, 0.3, 1.0):
                m = rng.random(n) < density
                want = [sum(1 for r in range(n) if m[r] and ids[r] == g) for g in group_ids]
                got = fo.counts(m, ids)
                assert got.dtype == np.int32 and got.tolist() == want
                words = fo.pack(np.flatnonzero(m), n)
                words[-1] |= np.uint32((0xFFFFFFFF << (n % 32)) & 0xFFFFFFFF) if n % 32 else np.uint32(0)   # tail bits never count
                assert fo.counts(words, ids, words=True).tolist() == want
            assert fo.counts(None, ids).tolist() == np.bincount(dense_of).tolist()
    b = fo.counts_batch([None, np.zeros(4, bool), np.array([1, 0, 0, 1], bool)], [9, 2, 2, 9])
    assert b.dtype == np.int32 and b.tolist() == [[2, 2], [0, 0], [0, 2]]
    row, vals = [3, 0, 5, 3, 1], ["a", "b", "c", "d", "e"]
    assert fo.facets(row, vals) == [{"value": "c", "count": 5}, {"value": "a", "count": 3}, {"value": "d", "count": 3}, {"value": "e", "count": 1}]
    assert [f["value"] for f in fo.facets(row, vals, min_count=0)] == ["c", "a", "d", "e", "b"]
    assert [f["value"] for f in fo.facets(row, vals, limit=2, min_count=3)] == ["c", "a"]


# ---- the service on its host side -------------------------------------------------------------------------------------------------
class StubMask:
    def __init__(self, rows, n, transient=False):
        self.bits = np.zeros(n, bool)
        self.bits[np.asarray(rows, np.int64)] = True
        self.rows, self.closed, self.transient = len(rows), False, transient

    def stats(self):
        return {"rows": self.rows, "bytes": 0}

    def close(self):
        self.closed = True


class StubGrouping:
    def __init__(self, group_of, max_nq):
        self.group_of, self.max_nq, self.closed = np.asarray(group_of), max_nq, False

    def stats(self):
        return {"groups": len(set(self.group_of.tolist())), "largest_group": 0, "bytes": 0}

    def close(self):
        self.closed = True


class StubIndex:
    """IcdIndex as the facets see it, answered by the oracle; every group_counts call is noted"""

    def __init__(self, n, max_nq):
        self.n, self.max_nq, self.closed, self.calls, self.made, self.fail = n, max_nq, False, [], [], None

    def rowmask(self, rows):
        self.made.append(len(rows))
        return StubMask(rows, self.n)

    def grouping(self, group_of, max_nq=None):
        assert len(group_of) == self.n
        return StubGrouping(group_of, max_nq)

    def group_counts(self, masks, grouping, on_device=False):
        assert 1 <= len(masks) <= self.max_nq and not grouping.closed and all(m is None or not m.closed for m in masks)
        self.calls.append(len(masks))
        if self.fail is not None:
            raise self.fail
        return fo.counts_batch([None if m is None else m.bits for m in masks], grouping.group_of)

    def close(self):
        self.closed = True


RECORDS = [{"code": c, "preferred_zh": t, "level": lv, "parent_code": p, "has_complication": hc, "main_code": None, "secondary_code": None,
            "category_path": path}
           for c, t, lv, p, hc, path in [
               ("A00", "霍乱", 1, "", False, "A00-A09 > A00"), ("A00.0", "霍乱，由于O1群霍乱弧菌", 2, "A00", False, "A00-A09 > A00"),
               ("A00.1", "埃尔托霍乱", 2, "A00", False, "A00-A09 > A00"), ("A01", "伤寒和副伤寒", 1, "", False, "A00-A09 > A01"),
               ("A01.0", "伤寒", 2, "A01", True, "A00-A09 > A01"), ("A01.1", "副伤寒甲", 2, "A01", False, "A00-A09 > A01"),
               ("A01.2", "副伤寒乙", 2, "A01", False, "A00-A09 > A01"), ("A01.3", "副伤寒丙", 2, "A01", True, "A00-A09 > A01"),
               ("A01.4", "副伤寒，未特指", 2, "A01", False, "A00-A09 > A01"), ("A15", "呼吸道结核", 1, "", False, "A15-A19 > A15"),
               ("A15.0", "肺结核", 2, "A15", False, "A15-A19 > A15"), ("B00", "疱疹病毒感染", 1, "", False, "")]]


@pytest.fixture()
def svc(tmp_path, monkeypatch):
    monkeypatch.setenv("MILVUS_DB_PATH", str(tmp_path / "db"))
    monkeypatch.setenv("MILVUS_COLLECTION_NAME", "facets")
    from rag_project_icd10_amd.services.milvus_service import MilvusService

    class Emb:
        def encode_query(self, t):
            return np.ones(64, np.float32) / 8

    class Small(MilvusService):
        FILTER_ON_DEVICE = False    # the host route: filter_rows -> index.rowmask
        TEXT_MATCH_ON_DEVICE = False

    s = Small(Emb())
    yield s
    s.disconnect()


def load(svc, max_nq=3):
    rng = np.random.default_rng(0)
    assert svc.insert_records(RECORDS, [rng.standard_normal(64).astype(np.float32) for _ in RECORDS]) is True
    svc._index = StubIndex(len(RECORDS), max_nq)
    svc._index_rows, svc._index_gen = svc.client.count, svc.client.generation
    return svc._index


def by_hand(svc, field, expr, limit=None, min_count=1):
    """the facet list from the host route's rows and a Counter over the field's values"""
    ids, values = svc._filter_columns().group_ids(field)
    rows = svc.filter_rows(expr) if expr else np.arange(svc.client.count)
    row = np.bincount(ids[rows], minlength=len(values))
    return fo.facets(row, values.tolist(), limit, min_count)


def test_empty_collection_answers_from_the_host(svc):
    assert svc.facet("level") == [] and svc.facet("category", "level == 2", limit=3) == []
    assert svc.facet_batch("code", ["", "level == 1"]) == [[], []] and svc.facet_batch("code", []) == []
    assert svc.facet_batch("code", ["", None], with_totals=True) == ([[], []], [0, 0])
    for bad in (lambda: svc.facet("nope"), lambda: svc.facet("level", "level =="), lambda: svc.facet("level", limit=0)):
        with pytest.raises(ValueError):      # a bad argument raises on an empty collection too
            bad()


def test_argument_checks(svc):
    index = load(svc)
    bad = [
        lambda: svc.facet("nope"), lambda: svc.facet(None), lambda: svc.facet(3), lambda: svc.facet("semantic_text"), lambda: svc.facet("vector"),
        lambda: svc.facet("level", "level =="), lambda: svc.facet("level", "nope == 1"), lambda: svc.facet("level", 7),
        lambda: svc.facet("level", limit=0), lambda: svc.facet("level", limit=-2), lambda: svc.facet("level", limit=True), lambda: svc.facet("level", limit=2.5),
        lambda: svc.facet("level", min_count=-1), lambda: svc.facet("level", min_count=True), lambda: svc.facet("level", min_count=None),
        lambda: svc.facet_batch("level", "level == 1"), lambda: svc.facet_batch("level", ["level == 1", "x"]), lambda: svc.facet_batch("nope", []),
    ]
    for i, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
            pytest.fail(f"case {i} did not raise")
    assert index.calls == [] and index.made == []      # every check came before the index was asked


def test_facets_over_a_stub_index(svc):
    index = load(svc)
    # ordering: count descending, equal counts in the values' ascending order
    assert svc.facet("level") == [{"value": 2, "count": 8}, {"value": 1, "count": 4}]
    assert svc.facet("parent_code") == [{"value": "A01", "count": 5}, {"value": "", "count": 4}, {"value": "A00", "count": 2}, {"value": "A15", "count": 1}]
    assert svc.facet("category") == [{"value": "A00-A09", "count": 9}, {"value": "A15-A19", "count": 2}, {"value": "B00", "count": 1}]
    assert svc.facet("has_complication", "level == 2") == [{"value": False, "count": 6}, {"value": True, "count": 2}]
    ties = svc.facet("code", 'code like "A01%"')
    assert [f["value"] for f in ties] == ["A01", "A01.0", "A01.1", "A01.2", "A01.3", "A01.4"] and {f["count"] for f in ties} == {1}
    assert all(type(f["count"]) is int for f in ties) and type(svc.facet("level")[0]["value"]) is int
    # min_count and limit
    assert svc.facet("parent_code", min_count=3) == svc.facet("parent_code")[:2]
    assert svc.facet("parent_code", limit=1) == svc.facet("parent_code")[:1] and svc.facet("parent_code", limit=99) == svc.facet("parent_code")
    zero = svc.facet("parent_code", "level == 1", min_count=0)
    assert zero == [{"value": "", "count": 4}, {"value": "A00", "count": 0}, {"value": "A01", "count": 0}, {"value": "A15", "count": 0}]
    assert svc.facet("parent_code", "level == 1", min_count=0, limit=2) == zero[:2]
    assert svc.facet("level", "level > 5") == [] and svc.facet("level", "level > 5", min_count=0) == [{"value": 1, "count": 0}, {"value": 2, "count": 0}]
    for field in ("level", "code", "parent_code", "has_complication", "category", "main_code"):
        for expr in ("", "level == 2", 'code like "A0%" and not has_complication == true', "level > 5"):
            for kw in ({}, {"limit": 2}, {"min_count": 2}, {"min_count": 0, "limit": 3}):
                assert svc.facet(field, expr, **kw) == by_hand(svc, field, expr, **kw), (field, expr, kw)
    # a batch: ONE _masks_for call, one group_counts call per max_nq masks, equal expressions share a mask, no filter is a NULL entry
    filters = ["level == 2", 'code like "A01%"', "", "level == 2", "level > 5", None, 'code like "A01%"']
    svc._clear_views()
    index.calls.clear(); index.made.clear()
    seen = []
    real = svc._masks_for
    svc._masks_for = lambda idx, exprs, nq: (seen.append(list(exprs)), real(idx, exprs, nq))[1]
    try:
        lists, totals = svc.facet_batch("parent_code", filters, with_totals=True)
    finally:
        del svc._masks_for
    assert len(seen) == 1 and seen[0] == ["level == 2", 'code like "A01%"', None, "level == 2", "level > 5", None, 'code like "A01%"']
    assert index.calls == [3, 3, 1] and index.made == [8, 6, 0]
    assert totals == [8, 6, 12, 8, 0, 12, 6]
    assert lists == [by_hand(svc, "parent_code", f) for f in filters] == [svc.facet("parent_code", f or "") for f in filters]
    assert svc.facet_batch("parent_code", filters, limit=1, min_count=2) == [l[:1] if l and l[0]["count"] >= 2 else [] for l in lists]
    # the grouping is the whole store's, made once per field
    assert len([g for g in svc.groupings() if g["field"] == "parent_code" and g["filter"] is None]) == 1


def test_masks_are_released_when_the_count_raises(svc):
    index = load(svc)
    own = [StubMask([1, 2], index.n, transient=True), None, StubMask([3], index.n)]   # a search's own mask, no filter, a cached one
    svc._masks_for = lambda idx, exprs, nq: own
    index.fail = RuntimeError("the device said no")
    with pytest.raises(RuntimeError, match="the device said no"):
        svc.facet_batch("level", ["level == 2", "", "level == 1"])
    assert own[0].closed and not own[2].closed and index.calls == [3]
    index.fail = None
    own[0] = StubMask([1, 2], index.n, transient=True)
    assert svc.facet_batch("level", ["level == 2", "", "level == 1"])[0] == [{"value": 2, "count": 2}] and own[0].closed


def test_facets_endpoint():
    from fastapi.testclient import TestClient
    from rag_project_icd10_amd.api import app as appmod

    class Mil:
        def __init__(self):
            self.seen = []

        def facet_batch(self, field, filters, limit=None, min_count=1, with_totals=False):
            self.seen.append((field, list(filters), limit, min_count, with_totals))
            if field == "nope":
                raise ValueError("field='nope': not one of ...")
            if field == "code":
                raise RuntimeError("boom")
            return [[{"value": np.int32(2), "count": 8}, {"value": np.int32(1), "count": 4}]], [12]

        def get_collection_stats(self):
            return {"num_entities": 3}

        def test_connection(self):
            return {"connected": True}

        def disconnect(self):
            return {}

    class Emb:
        def get_model_info(self):
            return {"loaded": True, "model_name": "stub"}

    mil = Mil()
    appmod.install_services(Emb(), mil, object())
    try:
        with TestClient(appmod.app) as client:
            r = client.post("/codes/facets", json={"field": "level", "filter": "level >= 1", "limit": 5, "min_count": 2})
            assert r.status_code == 200, r.text
            assert r.json() == {"field": "level", "total": 12, "facets": [{"value": 2, "count": 8}, {"value": 1, "count": 4}]}
            assert mil.seen == [("level", ["level >= 1"], 5, 2, True)]
            assert client.post("/codes/facets", json={"field": "level"}).status_code == 200 and mil.seen[-1] == ("level", [""], None, 1, True)
            assert client.post("/codes/facets", json={"field": "nope"}).status_code == 400
            assert client.post("/codes/facets", json={"field": "code"}).status_code == 500
            assert client.post("/codes/facets", json={}).status_code == 422          # no field at all: the model's own answer
    finally:
        appmod.install_services(None, None, None)
