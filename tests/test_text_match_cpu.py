"""TEXT_MATCH without a GPU: the grammar and its normalised key, the errors' positions and reasons, the host
matcher (SparseTextIndex.match_rows) against tests/text_match_oracle.py on the golden titles slice, composition through
Columns.select, and that every expression of the existing filter tests keeps its key."""
import os

import numpy as np
import pytest

import text_match_oracle as tmo
from conftest import GOLDEN
from rag_project_icd10_amd.services import filter_expr as fe, sparse_text


@pytest.fixture(scope="module")
def slice_():
    from rag_project_icd10_amd.tools.build_database import DatabaseBuilder
    recs = DatabaseBuilder.__new__(DatabaseBuilder).load_csv_data(os.path.join(GOLDEN, "csv_slice.csv"))   # (the CSV parser needs no services)
    titles = [str(r.get("preferred_zh") or "") for r in recs]
    tx = sparse_text.SparseTextIndex(titles)
    cols = fe.Columns.from_records(recs)
    return recs, titles, tx, cols


KEY = 'TEXT_MATCH(preferred_zh, "尿 尿病 病 糖 糖尿", minimum_should_match=1)'


def test_accepted_spellings_share_one_key():
    same = ['TEXT_MATCH(preferred_zh, "糖尿病")', "text_match(preferred_zh,'糖尿病')", 'Text_Match ( preferred_zh , "糖尿病" , MINIMUM_SHOULD_MATCH = 1 )',
            '(TEXT_MATCH(preferred_zh, "糖尿病", minimum_should_match=1))', 'TEXT_MATCH(preferred_zh, "糖尿病 糖尿病")',
            'TEXT_MATCH(preferred_zh, "  糖尿病，糖尿 ")']
    assert {fe.compile(e) for e in same} == {KEY}
    assert fe.compile(KEY) == KEY   # the key is an expression again
    assert fe.parse(KEY) == ("text_match", "preferred_zh", ("尿", "尿病", "病", "糖", "糖尿"), 1)
    assert fe.compile('TEXT_MATCH(preferred_zh, "E11.9 I10", minimum_should_match=2)') == 'TEXT_MATCH(preferred_zh, "e11.9 i10", minimum_should_match=2)'
    assert fe.compile('TEXT_MATCH(preferred_zh, "")') == 'TEXT_MATCH(preferred_zh, "", minimum_should_match=1)'
    both = fe.compile('level>=2 && text_match(preferred_zh, "糖尿病")')
    assert both == f"(level >= 2) and ({KEY})" and fe.compile(both) == both
    assert fe.compile('not TEXT_MATCH(preferred_zh, "糖尿病")') == f"not ({KEY})"
    assert fe.has_text_match(both) and not fe.has_text_match("level >= 2")


def test_device_shapes():
    assert fe.text_match_shape(KEY) == (None, "preferred_zh", ("尿", "尿病", "病", "糖", "糖尿"), 1)
    a = fe.text_match_shape('level >= 2 and TEXT_MATCH(preferred_zh, "糖尿病", minimum_should_match=3)')
    b = fe.text_match_shape('TEXT_MATCH(preferred_zh, "糖尿病", minimum_should_match=3) and level >= 2')
    assert a == b == ("level >= 2", "preferred_zh", ("尿", "尿病", "病", "糖", "糖尿"), 3)
    c = fe.text_match_shape('level >= 2 and TEXT_MATCH(preferred_zh, "a") and code like "E%"')
    assert c[0] == '(level >= 2) and (code like "E%")' and fe.compile(c[0]) == c[0]
    for host in ("level >= 2", 'level >= 2 or TEXT_MATCH(preferred_zh, "a")', 'not TEXT_MATCH(preferred_zh, "a")',
                 'TEXT_MATCH(preferred_zh, "a") and TEXT_MATCH(preferred_zh, "b")', 'level >= 2 and (level == 3 or TEXT_MATCH(preferred_zh, "a"))',
                 'level >= 2 and not TEXT_MATCH(preferred_zh, "a")'):
        assert fe.text_match_shape(host) is None, host


BAD = [
    ('TEXT_MATCH(nope, "x")', 11, "unknown field 'nope'"),
    ('TEXT_MATCH(code, "x")', 11, "carries no text index"),
    ('TEXT_MATCH(level, "x")', 11, "type mismatch"),
    ('TEXT_MATCH(preferred_zh, "x", minimum_should_match=0)', 51, "1 .. 64"),
    ('TEXT_MATCH(preferred_zh, "x", minimum_should_match=65)', 51, "1 .. 64"),
    ('TEXT_MATCH(preferred_zh, "x", minimum_should_match="2")', 51, "takes an int"),
    ('TEXT_MATCH(preferred_zh, "x", minimum_should_match=true)', 51, "takes an int"),
    ('TEXT_MATCH(preferred_zh "x")', 24, "expected ','"),
    ('TEXT_MATCH(preferred_zh, x)', 25, "quoted text"),
    ('TEXT_MATCH(preferred_zh, "x", min=2)', 33, "unexpected character"),
    ('TEXT_MATCH(preferred_zh, "x", minimum_should_match 2)', 30, "expected minimum_should_match="),
    ('TEXT_MATCH(preferred_zh, "x"', 28, "expected ')'"),
    ('TEXT_MATCH preferred_zh', 0, "unknown field 'TEXT_MATCH'"),
    ('PHRASE_MATCH(preferred_zh, "x")', 0, "unknown field 'PHRASE_MATCH'"),
]


@pytest.mark.parametrize("expr,pos,reason", BAD)
def test_errors_carry_position_and_reason(expr, pos, reason):
    with pytest.raises(ValueError) as e:
        fe.parse(expr)
    assert f"position {pos}:" in str(e.value) and reason in str(e.value), str(e.value)


def test_existing_expressions_keep_their_keys():
    """the expressions of tests/test_filter_expr_cpu.py parse to the keys they always had (recorded from the parent commit for the
    spellings listed there, and idempotent for every one of them)"""
    import test_filter_expr_cpu as old
    exprs = [c[0] for c in old.CASES] if hasattr(old, "CASES") else []
    exprs += ['level >= 2 and code like "E11%"', "(level>=2) && (code LIKE 'E11%')", '((level >= 2)) AND code like "E11%"']
    assert len(exprs) >= 3
    for e in exprs:
        k = fe.compile(e)
        assert "TEXT_MATCH" not in k and fe.compile(k) == k and fe.text_match_shape(e) is None and not fe.has_text_match(e)
    assert fe.compile("(level>=2) && (code LIKE 'E11%')") == '(level >= 2) and (code like "E11%")'
    assert fe.compile("level in [3, 1, 1]") == "level in [1, 3]" and fe.compile("NOT has_complication == TRUE") == "not (has_complication == true)"
    with pytest.raises(ValueError) as e:
        fe.parse("level = 1")
    assert "position 6: unexpected character" in str(e.value)


def test_match_rows_equals_the_oracle_on_the_golden_slice(slice_):
    recs, titles, tx, cols = slice_
    texts = ["糖尿病", "伤寒和副伤寒", "霍乱", "I10", "结核 肺", "zzzz", "", "肺结核 zzzz", titles[7], titles[40] + " " + titles[41]]
    some = False
    for text in texts:
        for m in (1, 2, "all"):
            want = tmo.match_text(titles, sparse_text.analyze, text, m)
            got = np.flatnonzero(tx.match_rows(text, m))
            assert np.array_equal(got, want), (text, m)
            assert np.array_equal(np.flatnonzero(tx.match_rows(sorted(set(sparse_text.analyze(text))), m)), want)
            known, total = tx.match_terms(text)
            if m != "all":
                assert np.array_equal(tmo.match_rows(tx.row_off, tx.terms, known, m), want)
            some |= 0 < len(want) < len(titles)
    assert some
    # an unknown term under "all" gives the empty set, though the known terms alone match rows
    assert tx.match_rows("结核", "all").any() and not tx.match_rows("结核 zzzz", "all").any()
    assert tx.match_terms("结核 zzzz")[1] == len(set(sparse_text.analyze("结核 zzzz")))
    for bad in (0, 65, 1.5, True, "any"):
        with pytest.raises(ValueError):
            tx.match_rows("结核", bad)


def test_more_than_64_known_terms_is_refused(slice_):
    recs, titles, tx, cols = slice_
    long_text = " ".join(titles[:40])
    assert len(tx.match_terms(tx.vocab[:64])[0]) == 64 and tx.match_rows(tx.vocab[:64], 1).any()   # exactly 64 is allowed
    with pytest.raises(ValueError):
        tx.match_rows(tx.vocab[:65], 1)
    with pytest.raises(ValueError) as e:
        tx.match_rows(long_text, 1)
    assert "at most 64" in str(e.value)
    cols.set_text_matcher("preferred_zh", tx.match_rows)
    escaped = long_text.replace('"', " ")
    with pytest.raises(ValueError):
        cols.select(f'TEXT_MATCH(preferred_zh, "{escaped}")')


def test_composition_through_columns(slice_):
    recs, titles, tx, cols = slice_
    fresh = fe.Columns.from_records(recs)
    with pytest.raises(ValueError) as e:
        fresh.select('TEXT_MATCH(preferred_zh, "结核")')
    assert "no sparse index on preferred_zh: call build_sparse_index" in str(e.value)
    with pytest.raises(ValueError):
        fe.select('TEXT_MATCH(preferred_zh, "结核")', {"preferred_zh": np.array(titles)})
    assert fe.compile('TEXT_MATCH(preferred_zh, "结核")')   # parsing and compile need no matcher
    cols.set_text_matcher("preferred_zh", tx.match_rows)
    n = len(titles)
    level = np.array([r.get("level", 1) for r in recs])
    a = tmo.match_text(titles, sparse_text.analyze, "结核", 1)
    b = tmo.match_text(titles, sparse_text.analyze, "伤寒", 2)
    assert 0 < len(a) < n and 0 < len(b) < n
    assert np.array_equal(cols.select('TEXT_MATCH(preferred_zh, "结核")'), a)
    assert np.array_equal(cols.select('not TEXT_MATCH(preferred_zh, "结核")'), np.setdiff1d(np.arange(n), a))
    assert np.array_equal(cols.select('level >= 2 and TEXT_MATCH(preferred_zh, "结核")'), a[level[a] >= 2])
    assert np.array_equal(cols.select('TEXT_MATCH(preferred_zh, "结核") or TEXT_MATCH(preferred_zh, "伤寒", minimum_should_match=2)'), np.union1d(a, b))
    assert np.array_equal(cols.select('TEXT_MATCH(preferred_zh, "")'), np.zeros(0, np.int64))


def test_text_match_expr_helper(slice_):
    recs, titles, tx, cols = slice_
    assert sparse_text.text_match_expr("preferred_zh", "糖尿病") == 'TEXT_MATCH(preferred_zh, "糖尿病", minimum_should_match=1)'
    e = sparse_text.text_match_expr("preferred_zh", '肺 "结核" \\ I10', "all")
    assert fe.parse(e) == ("text_match", "preferred_zh", ("i10", "核", "结", "结核", "肺"), 5)
    cols.set_text_matcher("preferred_zh", tx.match_rows)
    assert np.array_equal(cols.select(sparse_text.text_match_expr("preferred_zh", "肺结核", "all")), np.flatnonzero(tx.match_rows("肺结核", "all")))
    assert sparse_text.text_match_expr("preferred_zh", "", "all").endswith("minimum_should_match=1)")
    for bad in (0, 65, "most", 2.0, True):
        with pytest.raises(ValueError):
            sparse_text.text_match_expr("preferred_zh", "糖尿病", bad)
    with pytest.raises(ValueError):
        sparse_text.text_match_expr("preferred_zh", " ".join(titles[:40]), "all")
