"""The ordered select over row masks without a GPU: its host-only plan header under the host sanitizers, the
exported symbol and the ABI version, the numpy oracle against a brute-force walk, and MilvusService's scalar queries (query,
count(*), get, query_batch, query_iterator) on their host side - argument checks, the empty collection, and the paging logic over a
stub index that answers select_rows from the oracle."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import mask_select_oracle as mso
from conftest import ROOT
from rag_project_icd10_amd import _native


def test_plan_header_under_the_host_sanitizers(tmp_path):
    """tests/mask_select_plan_check.cpp: the host-only header that holds the segment and rank arithmetic, in a program of its own,
    with ASan and UBSan"""
    exe = str(tmp_path / "mask_select_plan_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                    os.path.join(ROOT, "rag_project_icd10_amd", "csrc"), os.path.join(ROOT, "tests", "mask_select_plan_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "mask select plan ok" in out.stdout


def test_symbol_abi_and_the_checks_that_need_no_device():
    lib = _native.load_library()
    assert hasattr(lib, "icd_rowmask_select") and "icd_rowmask_select" in _native.EXPORTED_SYMBOLS
    assert lib.icd_abi_version() == _native.ABI_VERSION == 6
    header = open(os.path.join(ROOT, "include", "icd_search.h"), encoding="utf-8").read()
    assert "#define ICD_SELECT_MAX_LIMIT 16384" in header and _native.SELECT_MAX_LIMIT == 16384
    plan = open(os.path.join(ROOT, "rag_project_icd10_amd", "csrc", "mask_select_plan.hpp"), encoding="utf-8").read()
    assert "hip/" not in plan and "__global__" not in plan                         # host only: no HIP header, no kernel
    assert _native.SELECT_SEGMENT_ROWS == 16384 and "MS_THREADS = 256" in plan and "MS_LANE_ROWS = 64" in plan
    total, taken, ids = np.zeros(2, np.int64), np.zeros(2, np.int32), np.zeros((2, 4), np.int64)
    table = (ctypes.c_void_p * 2)()
    call = lambda idx, nq, limit, tot=total: lib.icd_rowmask_select(idx, ctypes.cast(table, ctypes.c_void_p), nq, None, limit, ids.ctypes.data,   # noqa: E731
                                                                      None if tot is None else tot.ctypes.data, taken.ctypes.data, 0, None)
    assert call(None, 2, 0) == -1 and b"limit=0" in lib.icd_last_error()            # ICD_ERR_INVALID before the handle is looked at
    assert call(None, 2, 16385) == -1 and call(None, -1, 4) == -1 and call(None, 2, 4, None) == -1
    assert call(None, 2, 4) == -5                                                   # ICD_ERR_STATE: no index


def test_oracle_against_a_walk():
    rng = np.random.default_rng(5)
    for n in (1, 33, 200):
        for density in (0.0, 0.3, 1.0):
            m = rng.random(n) < density
            rows = [r for r in range(n) if m[r]]
            for offset in (0, 1, len(rows), len(rows) + 5):
                for limit in (1, 7, 300):
                    ids, total, taken = mso.select(m, n, offset, limit)
                    want = rows[offset:offset + limit]
                    assert total == len(rows) and taken == len(want) and ids.dtype == np.int64 and ids.shape == (limit,)
                    assert ids[:taken].tolist() == want and (ids[taken:] == -1).all()
    ids, total, taken = mso.select(None, 10, 8, 5)
    assert (ids.tolist(), total, taken) == ([8, 9, -1, -1, -1], 10, 2)
    b = mso.select_batch([None, np.zeros(10, bool)], 10, [8, 0], 5)
    assert b[0].shape == (2, 5) and b[1].tolist() == [10, 0] and b[2].dtype == np.int32 and b[2].tolist() == [2, 0]


# ---- the service on its host side -------------------------------------------------------------------------------------------------
class StubMask:
    def __init__(self, rows, n):
        self.bits = np.zeros(n, bool)
        self.bits[np.asarray(rows, np.int64)] = True
        self.rows, self.closed = len(rows), False

    def stats(self):
        return {"rows": self.rows, "bytes": 0}

    def close(self):
        self.closed = True


class StubIndex:
    """IcdIndex as the scalar queries see it, answered by the oracle; every select_rows call is noted"""

    def __init__(self, n, max_nq):
        self.n, self.max_nq, self.closed, self.calls = n, max_nq, False, []

    def rowmask(self, rows):
        return StubMask(rows, self.n)

    def select_rows(self, masks, limit, offsets=None, on_device=False):
        assert 1 <= len(masks) <= self.max_nq and 1 <= limit <= 16384
        offs = np.broadcast_to(np.asarray(0 if offsets is None else offsets, np.int64).reshape(-1), (len(masks),)) if np.size(offsets) <= 1 \
            else np.asarray(offsets, np.int64)
        assert (offs >= 0).all() and all(m is None or not m.closed for m in masks)
        self.calls.append((len(masks), limit, offs.tolist()))
        return mso.select_batch([None if m is None else m.bits for m in masks], self.n, offs, limit)

    def count_rows(self, masks):
        return self.select_rows(masks, 1)[1]

    def close(self):
        self.closed = True


RECORDS = [{"code": c, "preferred_zh": t, "level": lv, "parent_code": p, "has_complication": False, "main_code": None, "secondary_code": None}
           for c, t, lv, p in [("A00", "霍乱", 1, ""), ("A00.0", "霍乱，由于O1群霍乱弧菌", 2, "A00"), ("A00.1", "埃尔托霍乱", 2, "A00"),
                               ("A01", "伤寒和副伤寒", 1, ""), ("A01.0", "伤寒", 2, "A01"), ("A01.1", "副伤寒甲", 2, "A01"),
                               ("A01.2", "副伤寒乙", 2, "A01"), ("A01.3", "副伤寒丙", 2, "A01"), ("A01.4", "副伤寒，未特指", 2, "A01"),
                               ("A02", "其他沙门菌感染", 1, ""), ("A02.0", "沙门菌肠炎", 2, "A02")]]


@pytest.fixture()
def svc(tmp_path, monkeypatch):
    monkeypatch.setenv("MILVUS_DB_PATH", str(tmp_path / "db"))
    monkeypatch.setenv("MILVUS_COLLECTION_NAME", "scalar")
    from rag_project_icd10_amd.services.milvus_service import MilvusService

    class Emb:
        def encode_query(self, t):
            return np.ones(64, np.float32) / 8

    class Small(MilvusService):
        QUERY_WINDOW = 4            # (the walk of limit=None in windows, without 16384 records)
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


def test_empty_collection_answers_from_the_host(svc):
    assert svc.query('level == 2', limit=3) == [] and svc.query("") == [] and svc.count('code like "A%"') == 0 and svc.count() == 0
    assert svc.query(output_fields=["count(*)"]) == [{"count(*)": 0}]
    assert svc.query_batch(["", "level == 1"], 2) == [[], []] and svc.count_batch(["", "level == 1"]) == [0, 0]
    assert svc.query_batch([""], 2, with_totals=True) == ([[]], [0])
    assert svc.get([0, 1]) == [] and svc.query(ids=[3]) == []
    it = svc.query_iterator(batch_size=2, filter="level == 1")
    assert it.next() == [] and it.next() == []
    it.close()
    with pytest.raises(ValueError):          # a bad expression raises on an empty collection too
        svc.count("level ==")
    with pytest.raises(ValueError):
        svc.query("nope == 1", limit=2)


def test_argument_checks(svc):
    load(svc)
    bad = [
        lambda: svc.query("level == 1", limit=0), lambda: svc.query("level == 1", limit=-3), lambda: svc.query("level == 1", limit=True),
        lambda: svc.query("level == 1", limit=2.5), lambda: svc.query("level == 1", limit=2, offset=-1), lambda: svc.query("level == 1", offset=-1),
        lambda: svc.query("level == 1", limit=2, offset=3),                  # offset + limit above the window (4 here, 16384 in the product)
        lambda: svc.query("level == 1", limit=5),
        lambda: svc.query("level ==", limit=2), lambda: svc.query(7, limit=2), lambda: svc.count("code like"),
        lambda: svc.query("level == 1", output_fields=["count(*)"], limit=2),    # count(*) takes neither, as in Milvus
        lambda: svc.query("level == 1", output_fields=["count(*)"], offset=1),
        lambda: svc.query("level == 1", output_fields=["count(*)", "code"]),
        lambda: svc.query("level == 1", output_fields=["nope"], limit=2), lambda: svc.query("level == 1", output_fields="code", limit=2),
        lambda: svc.query("level == 1", ids=[1]), lambda: svc.query(ids=[1], limit=2), lambda: svc.query(ids=["A00"]), lambda: svc.get("A00"),
        lambda: svc.get([1.5]), lambda: svc.get([True]),
        lambda: svc.query_batch("level == 1", 2), lambda: svc.query_batch(["level == 1"], 2, offset=[0, 1]), lambda: svc.query_batch(["level =="], 2),
        lambda: svc.query_batch([], 0), lambda: svc.count_batch("level == 1"), lambda: svc.count_batch(["level == 1", "x"]),
        lambda: svc.query_iterator(batch_size=0), lambda: svc.query_iterator(batch_size=5), lambda: svc.query_iterator(batch_size=2, limit=-2),
        lambda: svc.query_iterator(filter="level =="), lambda: svc.query_iterator(output_fields=["nope"]),
    ]
    for i, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
            pytest.fail(f"case {i} did not raise")
    assert svc._index.calls == []            # every check came before the index was asked
    assert type(svc).__mro__[1].QUERY_WINDOW == 16384 == _native.SELECT_MAX_LIMIT


def test_queries_over_a_stub_index(svc):
    index = load(svc)
    recs = svc.client.records
    level2 = [i for i, r in enumerate(recs) if r["level"] == 2]
    a01 = [i for i, r in enumerate(recs) if r["code"].startswith("A01")]
    assert svc.filter_rows("level == 2").tolist() == level2 and len(level2) == 8
    # a window, the default fields, ascending id
    rows = svc.query("level == 2", limit=3, offset=1)
    assert [r["id"] for r in rows] == level2[1:4]
    assert set(rows[0]) == {"code", "preferred_zh", "has_complication", "main_code", "secondary_code", "level", "parent_code", "category_path",
                            "semantic_text", "id"}
    assert all(r[f] == recs[r["id"]].get(f) for r in rows for f in r if f != "id")
    assert svc.query("level == 2", limit=3, offset=1, output_fields=["code"]) == [{"code": recs[i]["code"], "id": i} for i in level2[1:4]]
    v = svc.query('code == "A01.0"', limit=1, output_fields=["vector", "code"])
    assert v[0]["code"] == "A01.0" and v[0]["vector"] == svc.client.matrix()[v[0]["id"]].tolist() and len(v[0]["vector"]) == 64
    # count(*), count, an empty filter, a filter of every row (a NULL mask: no rowmask is made), a filter of no row
    assert svc.query("level == 2", output_fields=["count(*)"]) == [{"count(*)": 8}] and svc.count("level == 2") == 8
    assert svc.count() == svc.count("") == svc.count("  ") == svc.count("level >= 1") == len(recs) and svc.count("level > 5") == 0
    assert svc.query("level > 5", limit=3) == [] and svc.query("level > 5") == []
    # limit=None: every row, walked in windows (4 rows here)
    index.calls.clear()
    assert [r["id"] for r in svc.query("level == 2")] == level2
    assert [c[1:] for c in index.calls] == [(4, [0]), (4, [4])]
    assert [r["id"] for r in svc.query("level == 2", offset=5)] == level2[5:]
    assert [r["id"] for r in svc.query("")] == list(range(len(recs)))
    # a batch: one select_rows call per max_nq masks, equal expressions share a mask, totals from the same call
    filters = ["level == 2", 'code like "A01%"', "", "level == 2", "level > 5", None, 'code like "A01%"']
    type(svc).QUERY_WINDOW = 16384   # (the fixture's own subclass: the product's window from here on)
    index.calls.clear()
    made = []
    real = index.rowmask
    index.rowmask = lambda rows: (made.append(len(rows)), real(rows))[1]
    svc._clear_views()
    lists, totals = svc.query_batch(filters, 2, offset=[0, 1, 9, 7, 0, 10, 5], with_totals=True)
    assert [c[0] for c in index.calls] == [3, 3, 1] and made == [8, 6, 0]
    assert totals == [8, 6, 11, 8, 0, 11, 6]
    assert [[r["id"] for r in l] for l in lists] == [level2[:2], a01[1:3], [9, 10], level2[7:], [], [10], a01[5:]]
    assert lists == [svc.query(f or "", limit=2, offset=o) for f, o in zip(filters, [0, 1, 9, 7, 0, 10, 5])]
    assert svc.count_batch(filters) == totals
    # get: the order asked for, unknown ids left out
    assert [r["id"] for r in svc.get([7, 99, 0, -1, 3])] == [7, 0, 3] and svc.get(4)[0]["code"] == "A01.0"
    assert svc.query(ids=[2, 50], output_fields=["code"]) == [{"code": "A00.1", "id": 2}]
    assert svc.get([]) == []


def test_iterator_pages_and_raises_after_a_mutation(svc):
    index = load(svc)
    recs = svc.client.records
    level2 = [i for i, r in enumerate(recs) if r["level"] == 2]
    it = svc.query_iterator(batch_size=3, filter="level == 2", output_fields=["code"])
    pages = []
    while True:
        page = it.next()
        if not page:
            break
        pages.append([r["id"] for r in page])
    assert pages == [level2[0:3], level2[3:6], level2[6:8]] and it.next() == []
    it.close()
    it = svc.query_iterator(batch_size=3, limit=4, filter="level == 2")
    assert [[r["id"] for r in it.next()] for _ in range(3)] == [level2[0:3], level2[3:4], []]
    it = svc.query_iterator(batch_size=4)                                     # no filter: every row
    assert [r["id"] for r in it.next()] == [0, 1, 2, 3]
    it0 = svc.query_iterator(batch_size=2, limit=0)
    assert it0.next() == []
    # a mutation of the store under a live iterator
    live = svc.query_iterator(batch_size=2, filter="level == 2")
    assert [r["id"] for r in live.next()] == level2[:2]
    assert svc.insert_records(RECORDS[:1], [np.ones(64, np.float32)]) is True
    with pytest.raises(RuntimeError):
        live.next()
    with pytest.raises(RuntimeError):
        it.next()
    live.close(); it.close()
    assert live.next() == []
    assert index.closed is False
