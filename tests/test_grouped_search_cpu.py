"""Grouping search, the parts that need no GPU: the group-id columns, argument validation, the request model, and the oracle
walk of tests/grouped_oracle.py against a brute force with hand-placed ties."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
from grouped_oracle import Ranking, expected

from rag_project_icd10_amd.services import filter_expr


@pytest.fixture(scope="module")
def records():
    return json.load(open(os.path.join(GOLDEN, "csv_records.json"), encoding="utf-8"))


def test_group_ids_are_ranks_of_the_sorted_distinct_values(records):
    cols = filter_expr.Columns.from_records(records)
    assert filter_expr.GROUP_FIELDS == filter_expr.FIELDS + ("category",) and len(filter_expr.FIELDS) == 8
    for field in filter_expr.GROUP_FIELDS:
        if field == "category":
            vals = [(r.get("category_path") or "").split(">")[0].strip() or r["code"] for r in records]
        elif field == "level":
            vals = [int(r.get("level", 1)) for r in records]
        elif field == "has_complication":
            vals = [bool(r.get("has_complication", False)) for r in records]
        else:
            vals = ["" if r.get(field) is None else str(r.get(field)) for r in records]
        distinct = sorted(set(vals))
        ids, values = cols.group_ids(field)
        assert ids.dtype == np.int32 and ids.shape == (len(records),) and values.tolist() == distinct, field
        assert [distinct[i] for i in ids] == vals, field
        assert cols.group_ids(field)[0] is ids   # cached
    # the rows without a parent (level 1) share the empty value: one group of their own
    ids, values = cols.group_ids("parent_code")
    top = [i for i, r in enumerate(records) if not r.get("parent_code")]
    assert top and values[0] == "" and set(ids[top].tolist()) == {0} and (ids == 0).sum() == len(top)
    # category: a code and its descendants share it; a level-1 row's is its own code
    ids, values = cols.group_ids("category")
    by_code = {r["code"]: values[ids[i]] for i, r in enumerate(records)}
    assert by_code["A00"] == "A00" and by_code["A00.0"] == "A00" and by_code["A00.001"] == "A00"
    # a record without a category_path falls back to its code
    odd = filter_expr.Columns.from_records([{"code": "Z99", "category_path": ""}, {"code": "Z99.1", "category_path": "Z99 > Z99.1"}, {"code": "Q1"}])
    ids, values = odd.group_ids("category")
    assert values.tolist() == ["Q1", "Z99"] and ids.tolist() == [1, 1, 0]


def test_grouping_argument_validation():
    filter_expr.check_grouping("level", 64, 2)
    filter_expr.check_grouping("category", 1, 128)
    with pytest.raises(ValueError, match="group_by_field='nope'.*category"):
        filter_expr.check_grouping("nope", 5, 1)
    with pytest.raises(ValueError, match="group_size=0.*>= 1"):
        filter_expr.check_grouping("level", 5, 0)
    with pytest.raises(ValueError, match="group_size=1.5"):
        filter_expr.check_grouping("level", 5, 1.5)
    with pytest.raises(ValueError, match="top_k=0"):
        filter_expr.check_grouping("level", 0, 1)
    with pytest.raises(ValueError, match=r"top_k \* group_size = 129 exceeds 128"):
        filter_expr.check_grouping("level", 43, 3)
    with pytest.raises(ValueError, match="exceeds 128"):
        filter_expr.check_grouping("level", 129, 1)
    # MilvusService validates before it touches the store (no index, no GPU needed)
    from rag_project_icd10_amd.services.milvus_service import MilvusService
    ms = MilvusService.__new__(MilvusService)
    ms.client = None
    q = np.zeros(8, np.float32)
    for kw in ({"group_by_field": "nope"}, {"group_by_field": "level", "group_size": 0}, {"group_by_field": "level", "group_size": 26},
               {"group_size": 2}):
        with pytest.raises(ValueError):
            ms.search(q, 5, **kw)
        with pytest.raises(ValueError):
            ms.search_batch(q[None], 5, **kw)


def test_query_request_grouping_fields():
    from pydantic import ValidationError
    from rag_project_icd10_amd.api.icd_models import QueryRequest
    r = QueryRequest(text="x")
    assert r.group_by_field is None and r.group_size == 1 and r.filter is None and r.top_k == 5
    r = QueryRequest(text="x", group_by_field="category", group_size=3)
    assert (r.group_by_field, r.group_size) == ("category", 3)
    for bad in ({"group_size": 0}, {"group_size": -1}, {"group_size": 129}, {"group_size": "many"}, {"group_by_field": 7}):
        with pytest.raises(ValidationError):
            QueryRequest(text="x", **bad)


def _brute(scores, group_of, k, s):
    """rules 1-3 by the book, one query: rank all rows by (score desc, id asc); a group ranks by its best row"""
    order = sorted(range(len(scores)), key=lambda i: (-float(scores[i]), i))
    members = {}
    for i in order:
        members.setdefault(int(group_of[i]), []).append(i)
    groups = sorted(members, key=lambda g: order.index(members[g][0]))[:k]
    return [i for g in groups for i in members[g][:s]]


def test_oracle_walk_against_a_brute_force_with_ties(oracle):
    n = 40
    rng = np.random.default_rng(5)
    scores = rng.integers(0, 6, (7, n)).astype(np.float32) / 4      # many exact ties inside and across groups
    scores[0, :] = 1.0                                              # everything ties: pure id order
    scores[1, [3, 17, 30]] = 9.0                                    # the best rows of three groups tie
    levels = rng.integers(1, 4, n).astype(np.int32)
    ids = np.stack([np.array(sorted(range(n), key=lambda i: (-float(r[i]), i)), np.int64) for r in scores])
    ranked = np.take_along_axis(scores, ids, 1)
    for group_of in (np.arange(n) // 5, (np.arange(n) * 7) % 3, np.arange(n), np.zeros(n, int), np.r_[np.zeros(37, int), [1, 1, 2]]):
        rk = Ranking(ranked, ids, group_of)
        for k, s in ((1, 1), (3, 1), (3, 2), (10, 3), (2, 40), (40, 1), (8, 5)):
            (raw, rid, lv, grp), (adj, araw, aid, alv, agrp) = expected(oracle, rk, levels, k, s)
            assert raw.shape == (7, k * s)
            for q in range(7):
                want = _brute(scores[q], group_of, k, s)
                m = len(want)
                assert rid[q, :m].tolist() == want and (rid[q, m:] == -1).all(), (k, s, q)
                assert raw[q, :m].tolist() == [scores[q, i] for i in want] and np.isneginf(raw[q, m:]).all()
                assert grp[q, :m].tolist() == [group_of[i] for i in want] and (grp[q, m:] == -1).all()
                assert lv[q, :m].tolist() == [levels[i] for i in want] and (lv[q, m:] == 0).all()
                # rule 4: adj = double(raw) * w[level], ONE stable descending sort of the list as handed back
                w = {1: 1.2, 2: 1.0, 3: 0.8}
                a = [float(scores[q, i]) * w[int(levels[i])] for i in want]
                order = sorted(range(m), key=lambda j: -a[j])
                assert aid[q, :m].tolist() == [want[j] for j in order] and adj[q, :m].tolist() == [a[j] for j in order]
                assert agrp[q, :m].tolist() == [group_of[want[j]] for j in order] and (agrp[q, m:] == -1).all()


def test_native_symbols_of_the_grouping_search():
    from rag_project_icd10_amd import _native
    for name in ("icd_grouping_create", "icd_grouping_destroy", "icd_grouping_stats", "icd_index_search_grouped"):
        assert name in _native.EXPORTED_SYMBOLS
    lib = _native.load_library()
    assert lib.icd_abi_version() == 6 and hasattr(lib, "icd_index_search_grouped")
    assert hasattr(_native.IcdIndex, "grouping") and hasattr(_native.IcdIndex, "search_grouped")


@pytest.mark.parametrize("id_base", [1000, 2**32 + 12345])
def test_a_ranking_shifted_by_id_base_gives_the_same_outputs_with_the_ids_shifted(oracle, id_base):
    n = 40
    rng = np.random.default_rng(6)
    scores = rng.integers(0, 6, (5, n)).astype(np.float32) / 4
    levels = rng.integers(1, 4, n).astype(np.int32)
    ids = np.stack([np.array(sorted(range(n), key=lambda i: (-float(r[i]), i)), np.int64) for r in scores])
    ranked = np.take_along_axis(scores, ids, 1)
    shift = lambda a: np.where(a >= 0, a + id_base, a)
    for group_of in (np.arange(n) // 5, (np.arange(n) * 7) % 3, np.arange(n)):
        for k, s in ((1, 1), (3, 2), (10, 3), (2, 40), (40, 1)):
            want = expected(oracle, Ranking(ranked, ids, group_of), levels, k, s)
            got = expected(oracle, Ranking(ranked, ids + id_base, group_of, id_base=id_base), levels, k, s, id_base=id_base)
            for j, (g, w) in enumerate(zip(got[0] + got[1], want[0] + want[1])):
                assert g.dtype == w.dtype and g.tobytes() == (shift(w) if w.dtype == np.int64 else w).tobytes(), (k, s, j)
    # a view: the view's own ranking (rows of the view, no base) through its row map, then the parent's id_base
    rows = np.arange(0, 2 * n, 2)
    plevels = rng.integers(1, 4, 2 * n).astype(np.int32)
    rk = Ranking(ranked, ids, np.arange(n) // 5)
    want = expected(oracle, rk, plevels, 3, 2, row_map=rows)
    got = expected(oracle, rk, plevels, 3, 2, row_map=rows, id_base=id_base)
    for j, (g, w) in enumerate(zip(got[0] + got[1], want[0] + want[1])):
        assert g.dtype == w.dtype and g.tobytes() == (shift(w) if w.dtype == np.int64 else w).tobytes(), j
