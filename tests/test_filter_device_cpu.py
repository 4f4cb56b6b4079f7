"""Filter programs for the device, the host side, no GPU: filter_expr.device_program against the host route
(filter_expr.select over the golden slice's Columns) through the numpy interpreter of the encoding (tests/filter_program_oracle.py),
its refusals, and icd_filter_program_check on malformed streams - through ctypes and in a program of its own under the host
sanitizers (tests/filter_program_check.cpp)."""
import os
import subprocess

import numpy as np
import pytest

import filter_program_oracle as fpo
import text_match_oracle as tmo
from conftest import GOLDEN
from rag_project_icd10_amd import _native
from rag_project_icd10_amd.services import filter_expr as fe
from rag_project_icd10_amd.services import sparse_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def slice_():
    from rag_project_icd10_amd.tools.build_database import DatabaseBuilder
    recs = DatabaseBuilder.__new__(DatabaseBuilder).load_csv_data(os.path.join(GOLDEN, "csv_slice.csv"))   # (the CSV parser needs no services)
    cols = fe.Columns.from_records(recs)
    tx = sparse_text.SparseTextIndex([r["preferred_zh"] for r in recs])
    cols.set_text_matcher("preferred_zh", tx.match_rows)
    return recs, cols, tx


EXPRESSIONS = [
    # every predicate kind
    "level == 2", "level != 3", "level < 2", "level <= 2", "level > 2", "level >= 2", "level > -1", "level < -5", "level >= 4000000000",
    "level in [1, 3]", "level not in [1,3]", "level in []",
    "has_complication == true", "has_complication == false", "has_complication != true", "has_complication in [true]",
    'code == "A01.0"', 'code == "nope"', 'code != "A00"', 'parent_code != ""', 'parent_code == "A01"', 'main_code == "A01.0"',
    'code in ["A00", "A01.0", "A01.001", "nope"]', 'code not in ["A00"]', "code in []", "code not in []",
    # like: prefix, suffix, infix, no %
    'code like "A0%"', 'code like "A01.0%"', 'code like "Z%"', 'secondary_code like "G%"', 'category_path like "A01 >%"',
    "code like '%.9'", "code like '%*'", 'preferred_zh like "%伤寒%"', 'preferred_zh like "%zzz%"', 'code like "A00"', 'preferred_zh like "%"',
    # or, not, nested
    'code like "A00%" or code like "A02%"', 'not code like "A0%"', '!(code like "A01%") and level >= 2',
    'code like "A00%" or code like "A01%" and level == 1', '(code like "A00%" or code like "A01%") and level == 1',
    'not (level == 1 and code like "A0%")', 'not not level == 2', 'not (not (level == 2 or not has_complication == true))',
    'NOT has_complication == true OR level IN [1] AND code LIKE "A02%"',
    '(level == 1 or (level == 2 and (code like "A0%" or (has_complication == true and (level >= 3 or code like "%9")))))',
    # TEXT_MATCH: alone, section 17's shape, under or / not, two of them
    'TEXT_MATCH(preferred_zh, "伤寒")', 'level >= 2 and TEXT_MATCH(preferred_zh, "霍乱")', 'TEXT_MATCH(preferred_zh, "zzzz")',
    'level == 1 or TEXT_MATCH(preferred_zh, "伤寒 肺炎", minimum_should_match=2)', 'not TEXT_MATCH(preferred_zh, "霍乱")',
    'TEXT_MATCH(preferred_zh, "伤寒") and not TEXT_MATCH(preferred_zh, "副伤寒", minimum_should_match=3)',
    'TEXT_MATCH(preferred_zh, "霍乱") or TEXT_MATCH(preferred_zh, "结核", minimum_should_match=64) or code like "A02%"',
    'TEXT_MATCH(preferred_zh, "霍乱 zzzz", minimum_should_match=3)',
]


def _text(tx):
    def fn(terms, m):
        hit = np.zeros(tx.n, bool)
        hit[tmo.match_rows(tx.row_off, tx.terms, terms, m)] = True
        return hit
    return fn


@pytest.mark.parametrize("expr", EXPRESSIONS)
def test_programs_select_what_the_host_route_selects(slice_, expr):
    recs, cols, tx = slice_
    prog = fe.device_program(expr, cols, {"preferred_zh": tx})
    assert prog is not None and prog.dtype == np.uint32, expr
    off, words = fe.pack_programs([prog])
    assert _native.filter_program_check(off, words, len(fe.DEVICE_COLUMNS), tx.vocab_size) is None
    got = fpo.run(prog, cols.device_columns(), _text(tx))
    want = fe.select(expr, cols)
    assert np.array_equal(got, want), (expr, len(got), len(want))


def test_the_slice_exercises_the_cases(slice_):
    recs, cols, tx = slice_
    sizes = {e: len(fe.select(e, cols)) for e in EXPRESSIONS}
    n = len(recs)
    assert sizes['code like "A0%"'] not in (0, n) and sizes["code like '%.9'"] > 0 and sizes['preferred_zh like "%伤寒%"'] > 0
    assert sizes['TEXT_MATCH(preferred_zh, "伤寒")'] > 0 and sizes["level in []"] == 0 and sizes["code not in []"] == n
    table = cols.device_columns()
    assert table.shape == (8, n) and table.dtype == np.int32 and table.flags.c_contiguous
    assert np.array_equal(table[fe.DEVICE_COLUMNS.index("code")], cols.group_ids("code")[0])
    assert np.array_equal(table[fe.DEVICE_COLUMNS.index("level")], cols["level"]) and set(np.unique(table[fe.DEVICE_COLUMNS.index("has_complication")])) <= {0, 1}


def nested(leaves):
    """`leaves` predicates nested to the right under alternating and / or: evaluated in the order written, the stack holds all of them"""
    out = f"level == {leaves}"
    for i in range(leaves - 1, 0, -1):
        out = f"level == {i} {'and' if i % 2 else 'or'} ({out})"
    return out


def test_refusals_give_none(slice_):
    recs, cols, tx = slice_
    text = {"preferred_zh": tx}
    assert fe.device_program(" or ".join(f"level == {i}" for i in range(16)), cols, text) is not None
    assert fe.device_program(" or ".join(f"level == {i}" for i in range(17)), cols, text) is None          # 17 leaves
    codes = sorted({r["code"] for r in recs})
    in_list = lambda k: "code in [" + ", ".join(f'"{c}"' for c in codes[:k]) + "]"   # noqa: E731
    assert fe.device_program(in_list(64), cols, text) is not None
    assert fe.device_program(in_list(65), cols, text) is None                                              # a 65-value set
    assert fe.device_program("not " + in_list(65), cols, text) is None
    assert fe.device_program(nested(8), cols, text) is not None
    assert fe.device_program(nested(9), cols, text) is None                                                # a stack depth of 9
    assert fe.device_program('TEXT_MATCH(preferred_zh, "伤寒")', cols, None) is None                        # no index on the field
    assert fe.device_program('level == 1 or TEXT_MATCH(preferred_zh, "伤寒")', cols, {}) is None
    five = " or ".join(f'TEXT_MATCH(preferred_zh, "{w}")' for w in ("伤寒", "霍乱", "结核", "肺炎", "感染"))
    assert fe.device_program(five, cols, text) is None                                                     # 5 TEXT leaves
    assert fe.device_program(" and ".join(["not not not not level == 1"] * 7), cols, text) is None         # 35 operations
    with pytest.raises(ValueError):
        fe.device_program("level >", cols, text)
    # a refused expression is still the host route's
    assert len(fe.select(in_list(65), cols)) == 65


def test_prefix_ranges_are_contiguous_or_refused():
    values = np.array(sorted(["", "A", "A0", "A00", "A01", "A1", "B", "é", "汉", "汉字"]), dtype=str)
    for p in ("A", "A0", "A00", "B", "C", "汉", "汉字x", ""):
        lo, hi = fe._prefix_range(values, p)
        assert [str(v) for v in values[lo:hi]] == [str(v) for v in values if str(v).startswith(p)], p
    with pytest.raises(fe._NoProgram):   # a range whose border value lacks the prefix is refused (np.unique's order never gives one)
        fe._prefix_range(np.array(["B", "A0", "A1"], dtype=str), "A")


R, S, T, AND, OR, NOT = 1, 2, 3, 4, 5, 6
MALFORMED = [
    ("a RANGE cut off", [R, 0, 1]),
    ("a SET cut off", [S | 3 << 8, 0, 1, 2]),
    ("a TEXT cut off", [T | 2 << 8 | 1 << 16, 5]),
    ("stack underflow: AND on one set", [R, 0, 0, 1, AND]),
    ("stack underflow: NOT on none", [NOT]),
    ("a leftover stack", [R, 0, 0, 1, R, 1, 0, 1]),
    ("an empty program", []),
    ("a column >= ncols", [R, 8, 0, 1]),
    ("a SET column >= ncols", [S | 1 << 8, 9, 1]),
    ("unsorted set ids", [S | 2 << 8, 0, 5, 5]),
    ("set ids unsorted as int32", [S | 2 << 8, 0, 1, 0xFFFFFFFF]),
    ("a term >= vocab", [T | 1 << 8 | 1 << 16, 100]),
    ("unsorted terms", [T | 2 << 8 | 1 << 16, 7, 3]),
    ("m = 0", [T | 1 << 8, 5]),
    ("m = 65", [T | 1 << 8 | 65 << 16, 5]),
    ("5 TEXT leaves", [T | 1 << 8 | 1 << 16, 5] * 5 + [OR] * 4),
    ("65 set ids", [S | 65 << 8, 0] + list(range(65))),
    ("17 leaves", [R, 0, 0, 1] + [R, 0, 0, 1, OR] * 16),
    ("9 sets on the stack", [R, 0, 0, 1] * 9 + [OR] * 8),
    ("33 operations", [R, 0, 0, 1] + [NOT] * 32),
    ("an unknown operation", [7]),
    ("stray bits on a RANGE", [R | 1 << 8, 0, 0, 1]),
    ("stray bits on a NOT", [R, 0, 0, 1, NOT | 1 << 16]),
]


@pytest.mark.parametrize("name,words", MALFORMED, ids=[m[0] for m in MALFORMED])
def test_the_checker_refuses_malformed_streams(name, words):
    msg = _native.filter_program_check([0, len(words)], words, 8, 100)
    assert msg, name
    good = [R, 0, 0, 1]   # ... also behind a good program
    assert _native.filter_program_check([0, 4, 4 + len(words)], good + words, 8, 100)


def test_the_checker_accepts_the_limits_and_reports_through_the_abi():
    lib = _native.load_library()
    full = [S | 64 << 8, 7] + list(range(64)) + [T | 64 << 8 | 64 << 16] + list(range(36, 100)) + [AND, NOT]
    # 16 leaves, 31 operations, 8 sets on the stack twice
    deep = [R, 0, 0x80000000, 0x7FFFFFFF] * 8 + [AND] * 7 + [R, 1, 5, 5] * 7 + [OR] * 7 + [R, 2, 0, 9, OR]
    off, words = fe.pack_programs([np.array(p, np.uint32) for p in (full, deep, [S, 0])])
    assert _native.filter_program_check(off, words, 8, 100) is None
    assert "sparse index" in _native.filter_program_check(off, words, 8, 0)            # a TEXT leaf without a vocabulary
    assert lib.icd_filter_program_check(off.ctypes.data, words.ctypes.data, 3, 8, 100, None, 0) == 0
    assert lib.icd_filter_program_check(off.ctypes.data, words.ctypes.data, 3, 7, 100, None, 0) == -1 and b"column 7" in lib.icd_last_error()
    assert lib.icd_filter_program_check(None, None, 1, 8, 100, None, 0) == -1
    bad_off = np.array([0, 4, 2], np.int64)
    assert "decrease" in _native.filter_program_check(bad_off, [R, 0, 0, 1], 8, 100)
    assert "start at" in _native.filter_program_check([1, 4], [R, 0, 0, 1], 8, 100)


def test_program_checker_under_the_host_sanitizers(tmp_path):
    """tests/filter_program_check.cpp: the host-only header that holds the checker, in a program of its own, with ASan and UBSan"""
    exe = str(tmp_path / "filter_program_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                    os.path.join(ROOT, "rag_project_icd10_amd", "csrc"), os.path.join(ROOT, "tests", "filter_program_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "filter program cases ok" in out.stdout


def test_produced_mask_layout_under_the_host_sanitizers(tmp_path):
    """tests/produced_mask_layout_check.cpp: the host-only header that lays out the block of a call's produced masks (sections 17.3
    and 18.3), in a program of its own, with ASan and UBSan"""
    exe = str(tmp_path / "produced_mask_layout_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                    os.path.join(ROOT, "rag_project_icd10_amd", "csrc"), os.path.join(ROOT, "tests", "produced_mask_layout_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "produced-mask layouts ok" in out.stdout
