"""icd_filter_rowmasks on the device against the host route: a produced mask word for word
(IcdRowMask.words() against icd_rowmask_pack of the oracle's rows) and its row count (icd_rowmask_stats). Raw programs are
interpreted by tests/filter_program_oracle.py (numpy over whole columns, TEXT leaves by tests/text_match_oracle.py); the service's
expressions by filter_expr.select, the host route itself. Integer output: no tolerance anywhere. Shapes sit around a mask word
(32 rows), a mask tile (128) and the kernel's tile (T rows, from the build)."""
import ctypes
import os

import numpy as np
import pytest

import filter_program_oracle as fpo
import text_match_oracle as tmo
from rag_project_icd10_amd import _native
from rag_project_icd10_amd.services import filter_expr as fe
from rag_project_icd10_amd.services import sparse_text

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DIM = 32
VOCAB = 80
R, S, T_, AND, OR, NOT = 1, 2, 3, 4, 5, 6
I32_MIN, I32_MAX = 0x80000000, 0x7FFFFFFF


def tile():
    return _native.sparse_tile_rows()


def shapes():
    T = tile()
    return [1, 31, 32, 33, 127, 128, 129, T - 1, T, T + 1, 2 * T + 5]


def make_columns(n, seed):
    """column 0: one distinct value; 1: two; 2: n distinct (a permutation); 3: signed values around 0 with both int32 ends"""
    rng = np.random.default_rng(seed)
    c3 = rng.integers(-5, 6, n)
    c3[rng.integers(0, n, 2)] = [-2 ** 31, 2 ** 31 - 1]
    return np.ascontiguousarray(np.stack([np.full(n, 7), rng.integers(0, 2, n), rng.permutation(n), c3]).astype(np.int32))


def make_rows(n, seed):
    """Term 0 in every row, term 1 in the rows around every tile border, term 2 in no row, terms 3 / 4 in the rows 5 | r, terms 5
    and 6 in disjoint rows, 7 .. 9 random; the four rows of every counter word hold 0 / 1 / 63 / 64 of the terms 10 .. 73"""
    rng = np.random.default_rng(seed)
    T, rows = tile(), np.arange(n)
    edge = np.unique(np.clip(np.concatenate([np.arange(b - 3, b + 3) for b in range(T, n + T, T)] + [[n - 1]]), 0, n - 1))
    r, t = [rows], [np.zeros(n, np.int64)]
    for rows_, term in ((edge, 1), (rows[rows % 5 == 0], 3), (rows[rows % 5 == 0], 4), (rows[rows % 4 == 1], 5), (rows[rows % 4 == 2], 6)):
        r.append(rows_); t.append(np.full(len(rows_), term))
    r.append(rng.integers(0, n, 2 * n)); t.append(rng.integers(7, 10, 2 * n))
    for phase, count in ((1, 1), (2, 63), (3, 64)):
        rr = rows[rows % 4 == phase]
        r.append(np.repeat(rr, count)); t.append(np.tile(np.arange(10, 10 + count), len(rr)))
    r, t = np.concatenate(r), np.concatenate(t)
    _, first = np.unique(r * VOCAB + t, return_index=True)
    r, t = r[first], t[first]
    row_off = np.zeros(n + 1, np.int64)
    np.add.at(row_off, r + 1, 1)
    return np.cumsum(row_off), t.astype(np.uint32), np.ones(len(t), np.float32)


def text(terms, m):
    return [T_ | len(terms) << 8 | m << 16] + list(terms)


def programs(n):
    """(name, words): every leaf kind alone, NOT of a full / an empty match, NOT NOT, empty and full ranges, sets of 0 / 1 / 64
    ids, 16 leaves at depth 8, a 64-term TEXT beside scalars, two and four TEXT leaves on the same counters"""
    full, none = [R, 0, 7, 8], [R, 0, 8, 8]
    q64 = list(range(10, 74))
    out = [
        ("a range", [R, 3, (-2) & 0xFFFFFFFF, 3]), ("a set", [S | 3 << 8, 3, (-4) & 0xFFFFFFFF, 0, 5]), ("a text", text([3, 4], 2)),
        ("not full", full + [NOT]), ("not empty", none + [NOT]), ("not not", [R, 1, 1, 2, NOT, NOT]), ("not not full", full + [NOT, NOT]),
        ("the empty range", none), ("an inverted range", [R, 2, 9, 3]), ("the full range", [R, 3, I32_MIN, I32_MAX]),
        ("the widest range misses INT32_MAX only", [R, 3, I32_MIN, I32_MAX, NOT]),
        ("one distinct value", full), ("two distinct values", [R, 1, 0, 1]), ("n distinct values", [R, 2, n // 3, n // 3 + 40]),
        ("set of 0", [S, 2]), ("set of 1", [S | 1 << 8, 2, n - 1]), ("set of 64", [S | 64 << 8, 2] + list(range(0, 192, 3))),
        ("set of both int32 ends", [S | 2 << 8, 3, I32_MIN, I32_MAX]), ("not a set of 64", [S | 64 << 8, 2] + list(range(1, 129, 2)) + [NOT]),
        ("16 leaves at depth 8", [R, 2, 0, n // 2] * 8 + [AND] * 7 + [R, 3, 0, 3] * 4 + [S | 2 << 8, 1, 0, 1] * 3 + [OR] * 7 + [R, 1, 1, 2, AND]),
        ("depth 8 of distinct leaves", sum(([R, 2, 10 * i, 10 * i + 7] for i in range(8)), []) + [OR] * 7),
        ("64 terms beside scalars", [R, 1, 1, 2] + text(q64, 63) + [AND, S | 1 << 8, 3, 0, OR]),
        ("64 terms, m 1 .. 64", text(q64, 1) + text(q64, 64) + [NOT, AND]),
        ("two texts", text([5], 1) + text([6], 1) + [OR]), ("two texts and", text([5], 1) + text([6], 1) + [AND]),
        ("m = 64 after counters filled to 64", text(q64, 1) + text(list(range(0, 64)), 64) + [OR]),
        ("m = 64 twice", text(q64, 64) + text(q64, 64) + [AND]),
        ("four texts", text([1], 1) + text(q64, 63) + [OR] + text([2], 1) + [OR] + text([0, 1, 5], 3) + [NOT, AND]),
        ("m above count", text([3, 4], 3)), ("a text of no term", text([], 1) + [NOT]), ("text, then scalars", text([0], 1) + [R, 1, 0, 1, AND, NOT]),
    ]
    return out


class Built:
    def __init__(self, n, seed, id_base=0, max_nq=512):
        rng = np.random.default_rng(seed)
        self.n = n
        self.index = _native.IcdIndex(rng.standard_normal((n, DIM), dtype=np.float32), rng.integers(1, 4, n).astype(np.int32), device=0,
                                      max_nq=max_nq, max_k=128, id_base=id_base, probe=False)
        self.rows = make_rows(n, seed)
        self.sp = self.index.sparse(*self.rows, VOCAB, max_nq=max_nq, max_k=128)
        self.table = make_columns(n, seed)
        self.cols = self.index.columns(self.table)
        self._text = {}

    def text(self, terms, m):   # (one oracle evaluation per distinct leaf of a shape)
        key = (tuple(int(t) for t in terms), int(m))
        if key not in self._text:
            hit = np.zeros(self.n, bool)
            hit[tmo.match_rows(self.rows[0], self.rows[1], key[0], key[1])] = True
            self._text[key] = hit
        return self._text[key]

    def want(self, words, base=None):
        rows = fpo.run(words, self.table, self.text)
        return rows if base is None else np.intersect1d(rows, base)

    def close(self):
        for h in (self.cols, self.sp, self.index):
            h.close()


def check(b, progs, bases=None, base_rows=None, sp="own"):
    off, words = fe.pack_programs([np.asarray(w, np.uint32) for _, w in progs])
    masks = b.index.filter_masks(b.cols, b.sp if sp == "own" else sp, off, words, bases)
    assert len(masks) == len(progs)
    for i, ((name, w), mask) in enumerate(zip(progs, masks)):
        want = b.want(w, None if base_rows is None else base_rows[i])
        got, exp = mask.words(), _native.pack_rowmask(want, b.n)
        assert got.dtype == exp.dtype and got.shape == exp.shape
        bad = np.flatnonzero(got != exp)
        assert bad.size == 0, f"program {i} ({name}): words {bad[:6].tolist()} differ: {got[bad[:3]]} vs {exp[bad[:3]]}"
        st = mask.stats()
        assert st["rows"] == len(want) and st["bytes"] >= got.nbytes, (name, st, len(want))
    return masks


@pytest.mark.parametrize("case", range(11))
def test_masks_equal_the_oracle(case):
    n = shapes()[case]
    b = Built(n, 700 + case)
    assert b.cols.stats() == {"ncols": 4, "rows": n, "bytes": 16 * n}
    progs = programs(n)
    masks = check(b, progs)
    by = {name: m for (name, _), m in zip(progs, masks)}
    # NOT: every row and no bit at or behind n (words() holds whole 128-row tiles: their tail must be 0)
    for name in ("not empty", "not not full"):
        w = by[name].words()
        assert by[name].stats()["rows"] == n and int(sum(bin(int(x)).count("1") for x in w)) == n, name
        assert not np.unpackbits(w.view(np.uint8), bitorder="little")[n:].any(), name
    for name in ("not full", "the empty range", "an inverted range", "set of 0", "m above count"):
        assert by[name].stats()["rows"] == 0 and not by[name].words().any(), name
    for m in masks:
        m.close()
    b.close()


def test_batches_of_one_and_three_hundred_with_an_id_base():
    n = 2 * tile() + 5
    b = Built(n, 11, id_base=5000)
    progs = programs(n)
    many = [progs[(7 * i) % len(progs)] for i in range(300)]
    check(b, many[17:18])
    masks = check(b, many)
    assert b.index.filter_masks(b.cols, None, np.zeros(1, np.int64), np.zeros(0, np.uint32)) == []
    # scalar programs need no sparse index
    scalar = [p for p in progs if not ("text" in p[0] or "terms" in p[0] or p[0].startswith("m "))]
    assert len(scalar) >= 15
    check(b, scalar, sp=None)
    del masks
    b.close()


def test_base_masks():
    n = tile() + 129
    b = Built(n, 21)
    rng = np.random.default_rng(3)
    progs = programs(n)
    nq = len(progs)
    some = np.sort(rng.choice(n, n // 3, replace=False)).astype(np.int64)
    m_some, m_empty = b.index.rowmask(some), b.index.rowmask(np.zeros(0, np.int64))
    check(b, progs, [None] * nq)                                   # an all-NULL table is no table
    mixed = [None if i % 3 == 0 else (m_some if i % 3 == 1 else m_empty) for i in range(nq)]
    mixed_rows = [None if i % 3 == 0 else (some if i % 3 == 1 else np.zeros(0, np.int64)) for i in range(nq)]
    check(b, progs, mixed, mixed_rows)
    check(b, progs, m_some, [some] * nq)                           # ONE mask for every query
    # a produced mask is a base like any other: NOT under a base stays inside the base
    first = check(b, [("a range", [R, 1, 0, 1])])
    inside = b.want([R, 1, 0, 1])
    again = check(b, [("not full", [R, 0, 8, 8, NOT]), ("two texts", text([5], 1) + text([6], 1) + [OR, NOT])], [first[0], first[0]], [inside, inside])
    assert again[0].stats()["rows"] == len(inside)
    b.close()


def _raw_call(b, progs, bases=None, idx_handle=None, cols_handle=None, sp_handle="own"):
    """the C entry itself: (status, the out_masks array it left), out_masks pre-filled with a non-NULL pattern"""
    lib = b.index._lib
    nq = len(progs)
    off, words = fe.pack_programs([np.asarray(w, np.uint32) for w in progs])
    out = (ctypes.c_void_p * max(nq, 1))(*([0xDEAD] * max(nq, 1)))
    tb = None if bases is None else (ctypes.c_void_p * nq)(*bases)
    rc = lib.icd_filter_rowmasks(b.index._h if idx_handle is None else idx_handle, b.cols._h if cols_handle is None else cols_handle,
                                 b.sp._h if sp_handle == "own" else sp_handle, off.ctypes.data, words.ctypes.data if words.size else off.ctypes.data,
                                 nq, None if tb is None else ctypes.cast(tb, ctypes.c_void_p), ctypes.cast(out, ctypes.c_void_p), None)
    return rc, [out[i] for i in range(nq)]


def test_errors_leave_every_out_mask_null():
    INVALID, UNSUPPORTED, STATE = -1, -4, -5
    b, other = Built(300, 31), Built(300, 32)
    good = [[R, 0, 7, 8], text([3], 1)]
    foreign = other.index.rowmask(np.arange(10, dtype=np.int64))
    dead_cols = b.index.columns(b.table)
    dead_cols.close()
    dead_mask = b.index.rowmask(np.arange(5, dtype=np.int64))
    dead_mask.close()
    cases = [
        ("columns of another index", dict(cols_handle=other.cols._h), INVALID),
        ("a sparse index of another index", dict(sp_handle=other.sp._h), INVALID),
        ("a base mask of another index", dict(bases=[None, foreign._h.value]), INVALID),
        ("no columns", dict(cols_handle=ctypes.c_void_p()), STATE),
        ("no index", dict(idx_handle=ctypes.c_void_p()), STATE),
        ("a TEXT leaf without a sparse index", dict(sp_handle=None), INVALID),
    ]
    for name, kw, want in cases:
        rc, out = _raw_call(b, good, **kw)
        assert rc == want and all(not p for p in out), (name, rc, out, b.index._lib.icd_last_error())
    for name, bad in (("stack underflow", [R, 0, 7, 8, AND]), ("a leftover stack", [R, 0, 7, 8] * 2), ("a column >= ncols", [R, 4, 0, 1]),
                      ("a term >= vocab", text([VOCAB], 1)), ("m = 0", [T_ | 1 << 8, 3]), ("a cut leaf", [S | 5 << 8, 0, 1]), ("empty", [])):
        rc, out = _raw_call(b, [good[0], bad, good[1]])
        assert rc == INVALID and all(not p for p in out), (name, rc, out)
    view = b.index.view(np.arange(0, 300, 2, dtype=np.int64))
    rc, out = _raw_call(b, good, idx_handle=view._h)
    assert rc == UNSUPPORTED and all(not p for p in out)   # a view as idx: mask the parent
    lib = b.index._lib
    probe = ctypes.c_void_p(0xDEAD)
    assert lib.icd_columns_create(view._h, b.table.ctypes.data, 4, ctypes.byref(probe)) == UNSUPPORTED and not probe.value
    assert lib.icd_columns_create(b.index._h, None, 4, ctypes.byref(probe)) == INVALID
    assert lib.icd_columns_create(b.index._h, b.table.ctypes.data, 0, ctypes.byref(probe)) == INVALID
    assert lib.icd_columns_stats(None, None, None, None) == STATE and lib.icd_columns_destroy(None) == STATE
    assert lib.icd_filter_rowmasks(b.index._h, b.cols._h, None, None, None, 1, None, None, None) == INVALID
    # the Python layer: closed partners and bad shapes raise before the library is asked
    off, words = fe.pack_programs([np.asarray(w, np.uint32) for w in good])
    with pytest.raises(_native.IcdError) as e:
        b.index.filter_masks(dead_cols, b.sp, off, words)
    assert e.value.code == STATE
    with pytest.raises(_native.IcdError):
        b.index.filter_masks(b.cols, b.sp, off, words, [dead_mask, None])
    with pytest.raises(ValueError):
        b.index.filter_masks(b.cols, b.sp, off[:-1], words)
    with pytest.raises(ValueError):
        b.index.filter_masks(b.cols, None, off, words)                 # the library's refusal of a TEXT leaf without a sparse index
    with pytest.raises(ValueError):
        b.index.columns(b.table[:, :-1])
    # the call works after all of these
    check(b, [("a range", good[0]), ("a text", good[1])])
    other.close(); b.close()


def test_masks_are_destroyed_alone_in_any_order_and_outlive_index_and_columns():
    b = Built(1000, 41)
    progs = programs(1000)[:14]
    off, words = fe.pack_programs([np.asarray(w, np.uint32) for _, w in progs])
    want = [_native.pack_rowmask(b.want(w), 1000) for _, w in progs]
    masks = b.index.filter_masks(b.cols, b.sp, off, words)
    for i in reversed(range(len(masks))):                 # reverse order; the survivors stay readable
        masks[i].close()
        assert all(np.array_equal(masks[j].words(), want[j]) for j in range(i))
    masks = b.index.filter_masks(b.cols, b.sp, off, words)
    order = np.random.default_rng(1).permutation(len(masks))
    for pos, i in enumerate(order):
        masks[i].close()
        for j in order[pos + 1:][:3]:
            assert np.array_equal(masks[j].words(), want[j])
    before = b.index.filter_masks(b.cols, b.sp, off, words)
    after = b.index.filter_masks(b.cols, b.sp, off, words)
    for m in before:                                      # masks before the index and the columns ...
        m.close()
    b.cols.close()
    assert all(np.array_equal(m.words(), w) for m, w in zip(after, want))
    b.sp.close(); b.index.close()                         # ... and after them: the masks keep no pointer into either
    assert all(np.array_equal(m.words(), w) for m, w in zip(after, want))
    assert after[1].stats()["rows"] == int(sum(bin(int(x)).count("1") for x in want[1]))
    for m in after:
        m.close()


def _bits(outs):
    return [(o.cpu().numpy() if hasattr(o, "cpu") else o).tobytes() for o in outs]


def test_searches_take_a_produced_mask_like_a_listed_one():
    n = tile() + 200
    b = Built(n, 51)
    index, sp = b.index, b.sp
    rng = np.random.default_rng(8)
    progs = [p for p in programs(n) if p[0] in ("a range", "a set", "a text", "not not", "16 leaves at depth 8", "four texts", "not full", "not empty")]
    nq = len(progs)
    off, words = fe.pack_programs([np.asarray(w, np.uint32) for _, w in progs])
    produced = index.filter_masks(b.cols, sp, off, words)
    listed = [index.rowmask(b.want(w)) for _, w in progs]
    dense = rng.standard_normal((nq, DIM), dtype=np.float32)
    assert _bits(index.search_masked(dense, 10, produced)) == _bits(index.search_masked(dense, 10, listed))
    sq = sparse_text.csr_from_pairs([(np.asarray(q, np.uint32), np.full(len(q), 1.5, np.float32)) for q in ([3, 4], [5, 6], [1], [0, 1, 5], [2], [7, 8, 9, 10], [0], [10, 11])])
    assert _bits(index.search_sparse(sp, *sq, 10, masks=produced)) == _bits(index.search_sparse(sp, *sq, 10, masks=listed))
    fusion = index.fusion(nq * 2)
    hq = rng.standard_normal((nq, 2, DIM), dtype=np.float32)
    two = lambda ms: [m for m in ms for _ in range(2)]   # noqa: E731
    assert _bits(index.search_hybrid(hq, [10, 7], 8, fusion, masks=two(produced))) == _bits(index.search_hybrid(hq, [10, 7], 8, fusion, masks=two(listed)))
    grouping = index.grouping((np.arange(n) % 13).astype(np.int32), max_nq=64)
    a = index.search_sparse(sp, *sq, 4, masks=produced, grouping=grouping, group_size=2)
    c = index.search_sparse(sp, *sq, 4, masks=listed, grouping=grouping, group_size=2)
    assert _bits(a) == _bits(c)
    for h in produced + listed + [grouping, fusion]:
        h.close()
    b.close()


# ---- the service ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def services(tmp_path_factory):
    mp = pytest.MonkeyPatch()
    mp.setenv("MILVUS_DB_PATH", str(tmp_path_factory.mktemp("db")))
    mp.setenv("MILVUS_COLLECTION_NAME", "icd10_filter_device")
    mp.setenv("EMBEDDING_MODEL_NAME", "shibing624/text2vec-base-chinese")
    mp.setenv("ICD_EMBEDDING_ALLOW_SYNTHETIC", "1")
    from rag_project_icd10_amd.tools.build_database import DatabaseBuilder
    b = DatabaseBuilder()
    b.initialize_services()
    recs = b.load_csv_data(os.path.join(GOLDEN, "csv_slice.csv"))
    assert b.vectorize_and_index(recs) is True
    yield {"ms": b.milvus_service, "es": b.embedding_service, "recs": recs}
    b.milvus_service.disconnect()
    mp.undo()


SCALAR = [
    'code like "A0%"', 'level >= 2 and code like "A01%"', 'code like "A00%" or code like "A02%"', 'not code like "A0%"',
    "code like '%.9' and level == 2", 'preferred_zh like "%伤寒%" or level == 1', 'code in ["A00", "A01.0", "nope"] or level < 2',
    'code not in ["A00"] and has_complication == false', 'not (level == 1 or (code like "A01%" and not has_complication == true))',
    'parent_code != "" and (level in [2] or secondary_code like "G%")', "level > -1", "level in []", 'main_code == "A01.0" or code like "A00"',
]
TEXTUAL = [
    'level == 1 or TEXT_MATCH(preferred_zh, "伤寒")', 'not TEXT_MATCH(preferred_zh, "霍乱")',
    'TEXT_MATCH(preferred_zh, "伤寒") and not TEXT_MATCH(preferred_zh, "副伤寒", minimum_should_match=3)',
    'TEXT_MATCH(preferred_zh, "霍乱") or TEXT_MATCH(preferred_zh, "结核")', 'code like "A0%" and (level >= 3 or TEXT_MATCH(preferred_zh, "zzzz 感染"))',
    '(level >= 2 and TEXT_MATCH(preferred_zh, "肺结核", minimum_should_match=2)) or code like "A00%"',
]
SECTION_17 = ['TEXT_MATCH(preferred_zh, "结核")', 'level >= 2 and TEXT_MATCH(preferred_zh, "伤寒")']
HOST_ONLY = [" or ".join(f"level == {i}" for i in range(17))]   # (17 leaves: device_program refuses it)


def test_service_routes_agree(services):
    ms, es, recs = services["ms"], services["es"], services["recs"]
    exprs = SCALAR + TEXTUAL + SECTION_17 + HOST_ONLY + [None, SCALAR[0]]
    assert len(exprs) >= 20
    titles = [r["preferred_zh"] for r in recs]
    vecs = np.asarray(es.encode_query_batch([titles[(7 * i) % len(titles)] for i in range(len(exprs))]), dtype=np.float32)
    calls = []
    real = ms._index.filter_masks
    ms._index.filter_masks = lambda *a, **k: (calls.append(len(a[2]) - 1), real(*a, **k))[1]
    try:
        device = ms.search_batch(vecs, 10, filter=exprs, filter_mode="mask")
    finally:
        del ms._index.filter_masks
    # ONE filter_masks call for the batch's fresh expressions, section 17's shapes among them; the refused one went to the host
    assert calls == [len(SCALAR) + len(TEXTUAL) + len(SECTION_17)]
    cached = {f["expression"] for f in ms.filter_masks()}
    full = {fe.compile("level > -1")}                     # (selects every row: passes no mask and is not cached, on either route)
    assert {fe.compile(e) for e in SCALAR} - full <= cached and not any("TEXT_MATCH" in k for k in cached)
    assert all(f["rows"] < len(recs) for f in ms.filter_masks())
    # the device masks against the host route's rows, bit for bit
    index = ms._index
    ms._clear_views()
    made = ms._masks_for(index, exprs, len(exprs))
    ms.FILTER_ON_DEVICE = False
    try:
        host_rows = [None if e is None else ms.filter_rows(e) for e in exprs]
        for e, m, rows in zip(exprs, made, host_rows):
            if m is None:
                assert rows is None or len(rows) == index.n, e
            else:
                assert np.array_equal(m.words(), _native.pack_rowmask(rows, index.n)) and m.stats()["rows"] == len(rows), e
        ms._release_masks(made)
        assert all(m is None or m.closed == (getattr(m, "transient", False)) for m in made)
        ms._clear_views()
        host = ms.search_batch(vecs, 10, filter=exprs, filter_mode="mask")
    finally:
        ms.FILTER_ON_DEVICE = True
    assert _bits(device) == _bits(host)
    assert any(len(r) not in (0, index.n) for r in host_rows if r is not None) and len(host_rows[SCALAR.index("level in []")]) == 0
    # the other entries that take masks: one expression, device route against host route
    answers = []
    for on in (True, False):
        ms.FILTER_ON_DEVICE = on
        ms._clear_views()
        try:
            e1, e2 = SCALAR[2], TEXTUAL[0]
            answers.append((ms.search(vecs[0], 5, filter=e1, filter_mode="mask"), ms.search(vecs[1], 5, filter=e2, filter_mode="mask"),
                            ms.search_text(titles[3], 5, filter=e2), ms.search_text(titles[3], 5, filter=e1),
                            ms.search_iterator(vecs[2], batch_size=4, filter=e1, filter_mode="mask").next(),
                            ms.search_batch(vecs[:3], 5, as_dicts=True, filter=TEXTUAL[2], filter_mode="mask")))
        finally:
            ms.FILTER_ON_DEVICE = True
    assert answers[0] == answers[1] and answers[0][0] and answers[0][1]
    assert answers[0][0] == ms.search(vecs[0], 5, filter=SCALAR[2])   # the default mode (a view) gives the same hits


def test_a_batch_is_one_filter_masks_call(services):
    """What _masks_for promises: the programs of ALL fresh expressions of a batch - scalar-only ones, ones that hold a TEXT_MATCH
    anywhere, section 17's shapes with an S the device takes - are ONE filter_masks call and no match_masks call. The same batch
    again finds the scalar-only masks in the cache and carries only the text-holding ones: their masks are the search's own."""
    ms, es, recs = services["ms"], services["es"], services["recs"]
    exprs = ['code like "A02%"', 'level == 2 and code like "A0%"',
             'level == 2 or TEXT_MATCH(preferred_zh, "霍乱")', 'not TEXT_MATCH(preferred_zh, "结核")',
             'TEXT_MATCH(preferred_zh, "伤寒")', 'level >= 2 and TEXT_MATCH(preferred_zh, "感染")']
    text = [fe.has_text_match(e) for e in exprs]
    assert text == [False, False, True, True, True, True]
    assert [fe.text_match_shape(e) is not None for e in exprs] == [False, False, False, False, True, True]
    assert len({fe.compile(e) for e in exprs}) == len(exprs) and ms.FILTER_ON_DEVICE and ms.TEXT_MATCH_ON_DEVICE
    titles = [r["preferred_zh"] for r in recs]
    vecs = np.asarray(es.encode_query_batch([titles[(5 * i) % len(titles)] for i in range(len(exprs))]), dtype=np.float32)
    index = ms._ready_index()
    ms._clear_views()   # (nothing cached)
    assert ms.filter_masks() == []
    calls = {"match_masks": [], "filter_masks": []}
    real_match, real_filter = index.match_masks, index.filter_masks
    index.match_masks = lambda *a, **k: (calls["match_masks"].append(len(a[3])), real_match(*a, **k))[1]
    index.filter_masks = lambda *a, **k: (calls["filter_masks"].append(len(a[2]) - 1), real_filter(*a, **k))[1]
    try:
        first = ms.search_batch(vecs, 10, filter=exprs, filter_mode="mask")
        assert calls == {"match_masks": [], "filter_masks": [len(exprs)]}
        second = ms.search_batch(vecs, 10, filter=exprs, filter_mode="mask")
    finally:
        del index.match_masks, index.filter_masks
    own = sum(text)   # (has_text_match with TEXT_MATCH_ON_DEVICE on: the `own` rule - never read from the cache, never entered)
    assert calls == {"match_masks": [], "filter_masks": [len(exprs), own]}
    assert {f["expression"] for f in ms.filter_masks()} == {fe.compile(e) for e, t in zip(exprs, text) if not t}
    assert _bits(first) == _bits(second)


def test_endpoints_take_device_filters(services):
    # (last of the module: the app's lifespan disconnects the installed services when the client closes)
    from fastapi.testclient import TestClient
    from rag_project_icd10_amd.api import app as appmod
    from rag_project_icd10_amd.services.multi_diagnosis_service import MultiDiagnosisService
    ms, es, recs = services["ms"], services["es"], services["recs"]
    expr = 'code like "A01%" or TEXT_MATCH(preferred_zh, "霍乱")'
    ms.FILTER_ON_DEVICE = False
    allowed = {recs[i]["code"] for i in ms.filter_rows(expr)}
    ms.FILTER_ON_DEVICE = True
    ms._clear_views()
    assert allowed
    appmod.install_services(es, ms, MultiDiagnosisService(es, ms))
    try:
        with TestClient(appmod.app) as client:
            bodies = []
            for on in (True, False):
                ms.FILTER_ON_DEVICE = on
                ms._clear_views()
                r = client.post("/query", json={"text": "霍乱，伤寒；副伤寒", "top_k": 3, "filter": expr, "filter_mode": "mask"})
                h = client.post("/hybrid_query", json={"texts": ["伤寒", "副伤寒"], "top_k": 5, "req_limit": 20, "sparse": True, "filter": expr})
                assert r.status_code == 200 and r.json()["candidates"], r.text
                assert h.status_code == 200 and h.json()["candidates"], h.text
                assert all(c["code"] in allowed for m in r.json()["diagnosis_matches"] for c in m["candidates"])
                assert all(c["code"] in allowed for c in h.json()["candidates"])
                bodies.append(([c["code"] for m in r.json()["diagnosis_matches"] for c in m["candidates"]], [c["code"] for c in h.json()["candidates"]]))
            assert bodies[0] == bodies[1]
    finally:
        ms.FILTER_ON_DEVICE = True
        appmod.install_services(None, None, None)
