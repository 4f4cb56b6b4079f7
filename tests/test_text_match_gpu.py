"""icd_sparse_match_rowmasks on the device against tests/text_match_oracle.py: the produced masks word for
word (IcdRowMask.words() against icd_rowmask_pack of the oracle's rows) and their row counts (icd_rowmask_stats). Integer output:
no tolerance anywhere. Shapes sit around a mask word (32 rows), a mask tile (128) and the kernel's tile (T rows, from the build).
The vocabularies 1 and 37 cannot hold a query of 64 terms, so the 64-term query and the byte-carry rows use a third one, 80."""
import ctypes
import os

import numpy as np
import pytest

import text_match_oracle as tmo
from rag_project_icd10_amd import _native
from rag_project_icd10_amd.services import filter_expr, sparse_text

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DIM = 32


def tile():
    return _native.sparse_tile_rows()


def make_rows(n, vocab, seed):
    """Term 0 in EVERY row. Vocabulary 37: term 1 in the rows that straddle every tile boundary (and the last row), term 2 in no
    row, terms 3 and 4 in the same rows, terms 5 and 6 in disjoint rows, the rest random. Vocabulary 80: also the four rows of
    every counter word hold 0 / 1 / 63 / 64 of the terms 10 .. 73 (a byte that carried would show in its neighbour)."""
    rng = np.random.default_rng(seed)
    T = tile()
    rows = np.arange(n)
    r, t = [rows], [np.zeros(n, np.int64)]
    if vocab >= 37:
        edge = np.unique(np.clip(np.concatenate([np.arange(b - 3, b + 3) for b in range(T, n + T, T)] + [[n - 1]]), 0, n - 1))
        for rows_, term in ((edge, 1), (rows[rows % 5 == 0], 3), (rows[rows % 5 == 0], 4), (rows[rows % 4 == 1], 5), (rows[rows % 4 == 2], 6)):
            r.append(rows_); t.append(np.full(len(rows_), term))
        m = 3 * n
        r.append(rng.integers(0, n, m)); t.append(rng.integers(7, 10 if vocab >= 80 else vocab, m))
    if vocab >= 80:
        for phase, count in ((1, 1), (2, 63), (3, 64)):
            rr = rows[rows % 4 == phase]
            r.append(np.repeat(rr, count)); t.append(np.tile(np.arange(10, 10 + count), len(rr)))
    r, t = np.concatenate(r), np.concatenate(t)
    _, first = np.unique(r * vocab + t, return_index=True)
    r, t = r[first], t[first]
    row_off = np.zeros(n + 1, np.int64)
    np.add.at(row_off, r + 1, 1)
    return np.cumsum(row_off), t.astype(np.uint32), np.ones(len(t), np.float32)


def make_queries(vocab, extra=0, seed=5):
    """[(terms, m)]: 0 terms, 1 term, a term in every row, straddling a tile boundary, with empty postings, two terms sharing all
    rows / none, the whole vocabulary (64 terms at vocabulary 80), each at m = 1, 2, its number of terms and that + 1"""
    rng = np.random.default_rng(seed)
    qs = [[], [0]]
    if vocab >= 37:
        qs += [[1], [2], [3, 4], [5, 6], [1, 2, 3], [0, 1, 2, 3, 4, 5, 6], list(range(min(vocab, 37)))]
    if vocab >= 80:
        qs += [list(range(10, 74)), list(range(0, 64)), list(range(16, 80))]
    for _ in range(extra):
        qs.append(sorted(rng.choice(vocab, int(rng.integers(1, min(vocab, 9) + 1)), replace=False).tolist()))
    out = []
    for q in qs:
        for m in sorted({1, 2, max(len(q), 1), min(len(q) + 1, 64)}):
            out.append((q, m))
    return out


def build(n, vocab, seed, id_base=0, max_nq=512):
    rng = np.random.default_rng(seed)
    corpus = rng.standard_normal((n, DIM), dtype=np.float32)
    levels = rng.integers(1, 4, n).astype(np.int32)
    index = _native.IcdIndex(corpus, levels, device=0, max_nq=max_nq, max_k=128, id_base=id_base, probe=False)
    rows = make_rows(n, vocab, seed)
    return index, index.sparse(*rows, vocab, max_nq=max_nq, max_k=128), rows, levels


def csr(queries):
    return sparse_text.csr_from_pairs([(np.asarray(q, np.uint32), np.ones(len(q), np.float32)) for q, _ in queries])[:2], [m for _, m in queries]


def check(index, sp, rows, queries, bases=None, base_rows=None):
    (q_off, q_terms), mm = csr(queries)
    masks = index.match_masks(sp, q_off, q_terms, mm, bases)
    assert len(masks) == len(queries)
    for i, ((q, m), mask) in enumerate(zip(queries, masks)):
        want = tmo.match_rows(rows[0], rows[1], q, m, None if base_rows is None else base_rows[i])
        got = mask.words()
        exp = _native.pack_rowmask(want, index.n)
        assert got.dtype == exp.dtype and got.shape == exp.shape
        bad = np.flatnonzero(got != exp)
        assert bad.size == 0, f"query {i} terms {q[:8]} m={m}: words {bad[:6].tolist()} differ: {got[bad[:3]]} vs {exp[bad[:3]]}"
        st = mask.stats()
        assert st["rows"] == len(want) and st["bytes"] >= got.nbytes, (i, st, len(want))
    return masks


def shapes():
    T = tile()
    return [1, 31, 32, 33, 127, 128, 129, T - 1, T, T + 1, 2 * T + 5]


@pytest.mark.parametrize("vocab", [1, 37])
@pytest.mark.parametrize("case", range(11))
def test_masks_equal_the_oracle(case, vocab):
    n = shapes()[case]
    index, sp, rows, _ = build(n, vocab, 300 + case)
    queries = make_queries(vocab, extra=3)
    masks = check(index, sp, rows, queries)
    # an empty answer is the empty mask: m above the number of terms, no term at all, a term with no postings
    assert masks[0].stats()["rows"] == 0 and not masks[0].words().any()
    for m in masks:
        m.close()
    sp.close(); index.close()


@pytest.mark.parametrize("n_of", [lambda T: 33, lambda T: T + 1, lambda T: 2 * T + 5])
def test_sixty_four_terms_and_no_byte_carry(n_of):
    """rows 4 j .. 4 j + 3 share one counter word and hold 0 / 1 / 63 / 64 of the query's 64 terms at once"""
    n = n_of(tile())
    index, sp, rows, _ = build(n, 80, 77)
    q64 = list(range(10, 74))
    queries = [(q64, m) for m in (1, 2, 62, 63, 64)] + make_queries(80)
    masks = check(index, sp, rows, queries)
    r = np.arange(n)
    assert masks[0].stats()["rows"] == int((r % 4 != 0).sum())          # m = 1: counts 1, 63, 64
    assert masks[1].stats()["rows"] == int((r % 4 >= 2).sum())          # m = 2: counts 63, 64
    assert masks[3].stats()["rows"] == int((r % 4 >= 2).sum())          # m = 63
    assert masks[4].stats()["rows"] == int((r % 4 == 3).sum())          # m = 64: only the full rows
    sp.close(); index.close()


def test_batches_of_one_and_three_hundred_with_an_id_base():
    T = tile()
    n = 2 * T + 5
    index, sp, rows, _ = build(n, 37, 11, id_base=5000)
    base = make_queries(37, extra=40, seed=9)
    queries = [base[i % len(base)] for i in range(300)]
    assert len({m for _, m in queries}) >= 4
    check(index, sp, rows, queries[17:18])
    masks = check(index, sp, rows, queries)
    assert index.match_masks(sp, np.zeros(1, np.int64), np.zeros(0, np.uint32), []) == []
    del masks
    sp.close(); index.close()


def test_base_masks():
    T = tile()
    n = T + 129
    index, sp, rows, _ = build(n, 37, 21)
    rng = np.random.default_rng(3)
    queries = make_queries(37, extra=2)
    nq = len(queries)
    some = np.sort(rng.choice(n, n // 3, replace=False)).astype(np.int64)
    m_some, m_empty = index.rowmask(some), index.rowmask(np.zeros(0, np.int64))
    check(index, sp, rows, queries, None)
    check(index, sp, rows, queries, [None] * nq)                                   # an all-NULL table is no table
    mixed = [None if i % 3 == 0 else (m_some if i % 3 == 1 else m_empty) for i in range(nq)]
    mixed_rows = [None if i % 3 == 0 else (some if i % 3 == 1 else np.zeros(0, np.int64)) for i in range(nq)]
    check(index, sp, rows, queries, mixed, mixed_rows)
    check(index, sp, rows, queries, m_some, [some] * nq)                           # ONE mask for every query
    # a base that removes exactly the matching rows leaves nothing; its complement leaves everything
    q, m = [3, 4], 2
    hit = tmo.match_rows(rows[0], rows[1], q, m)
    assert 0 < len(hit) < n
    rest = np.setdiff1d(np.arange(n), hit)
    got = check(index, sp, rows, [(q, m), (q, m)], [index.rowmask(rest), index.rowmask(hit)], [rest, hit])
    assert got[0].stats()["rows"] == 0 and got[1].stats()["rows"] == len(hit)
    # a produced mask is a base like any other
    again = check(index, sp, rows, [([0], 1)], [got[1]], [hit])
    assert again[0].stats()["rows"] == len(hit)
    sp.close(); index.close()


def _raw_call(index, sp, q_off, q_terms, mm, bases=None, sp_handle=None, idx_handle=None):
    """the C entry itself: (status, the out_masks array it left), out_masks pre-filled with a non-NULL pattern"""
    lib = index._lib
    nq = len(mm)
    out = (ctypes.c_void_p * max(nq, 1))(*([0xDEAD] * max(nq, 1)))
    q_off, q_terms, mm = np.asarray(q_off, np.int64), np.asarray(q_terms, np.uint32), np.asarray(mm, np.int32)
    b = None
    if bases is not None:
        b = (ctypes.c_void_p * nq)(*[None if x is None else x for x in bases])
    rc = lib.icd_sparse_match_rowmasks(index._h if idx_handle is None else idx_handle, sp._h if sp_handle is None else sp_handle,
                                       q_off.ctypes.data, q_terms.ctypes.data if q_terms.size else q_off.ctypes.data, mm.ctypes.data, nq, 0,
                                       None if b is None else ctypes.cast(b, ctypes.c_void_p), ctypes.cast(out, ctypes.c_void_p), None)
    return rc, [out[i] for i in range(nq)]


def test_errors_leave_every_out_mask_null():
    INVALID, UNSUPPORTED, STATE = -1, -4, -5
    index, sp, rows, _ = build(300, 80, 31)
    other, sp_other, _, _ = build(300, 80, 32)
    ok_off, ok_terms = [0, 2, 3], [1, 5, 7]
    cases = [
        ("unsorted terms", dict(q_off=[0, 2, 3], q_terms=[5, 1, 7], mm=[1, 1]), INVALID),
        ("a repeated term", dict(q_off=[0, 2, 3], q_terms=[5, 5, 7], mm=[1, 1]), INVALID),
        ("a term at the vocabulary's end", dict(q_off=[0, 2, 3], q_terms=[1, 80, 7], mm=[1, 1]), INVALID),
        ("65 terms", dict(q_off=[0, 65, 66], q_terms=list(range(65)) + [3], mm=[1, 1]), INVALID),
        ("offsets that decrease", dict(q_off=[0, 2, 1], q_terms=[1, 5, 7], mm=[1, 1]), INVALID),
        ("offsets not from 0", dict(q_off=[1, 2, 3], q_terms=[1, 5, 7], mm=[1, 1]), INVALID),
        ("min_match 0", dict(q_off=ok_off, q_terms=ok_terms, mm=[1, 0]), INVALID),
        ("min_match 65", dict(q_off=ok_off, q_terms=ok_terms, mm=[65, 1]), INVALID),
        ("a sparse index of another index", dict(q_off=ok_off, q_terms=ok_terms, mm=[1, 1], sp_handle=sp_other._h), INVALID),
        ("no sparse index", dict(q_off=ok_off, q_terms=ok_terms, mm=[1, 1], sp_handle=ctypes.c_void_p()), STATE),
        ("no index", dict(q_off=ok_off, q_terms=ok_terms, mm=[1, 1], idx_handle=ctypes.c_void_p()), STATE),
    ]
    foreign = other.rowmask(np.arange(10, dtype=np.int64))
    cases.append(("a base mask of another index", dict(q_off=ok_off, q_terms=ok_terms, mm=[1, 1], bases=[None, foreign._h.value]), INVALID))
    for name, kw, want in cases:
        rc, out = _raw_call(index, sp, **kw)
        assert rc == want and all(not p for p in out), (name, rc, out, index._lib.icd_last_error())
    view = index.view(np.arange(0, 300, 2, dtype=np.int64))
    rc, out = _raw_call(index, sp, ok_off, ok_terms, [1, 1], idx_handle=view._h)
    assert rc == UNSUPPORTED and all(not p for p in out)   # a view as idx: mask the parent
    lib = index._lib
    assert lib.icd_sparse_match_rowmasks(index._h, sp._h, None, None, None, 1, 0, None, None, None) == INVALID
    assert lib.icd_rowmask_read(None, None, 0) == STATE
    good = index.match_masks(sp, ok_off, ok_terms, [1, 1])
    short = np.zeros(2, np.uint32)
    assert lib.icd_rowmask_read(good[0]._h, short.ctypes.data, 2) == INVALID and lib.icd_rowmask_read(good[0]._h, None, 100) == INVALID
    # the Python layer: closed partners and bad shapes raise before the library is asked
    closed = index.rowmask(np.arange(5, dtype=np.int64)); closed.close()
    with pytest.raises(_native.IcdError) as e:
        index.match_masks(sp, ok_off, ok_terms, [1, 1], [closed, None])
    assert e.value.code == STATE
    with pytest.raises(ValueError):
        index.match_masks(sp, ok_off, ok_terms, [1])
    with pytest.raises(ValueError):
        index.match_masks(sp, ok_off, [5, 1, 7], [1, 1])
    with pytest.raises(_native.IcdError):
        good[0].close(); good[0].words()
    # icd_rowmask_read serves a mask made from a row list too
    listed = index.rowmask(np.array([0, 31, 32, 299], np.int64))
    assert np.array_equal(listed.words(), _native.pack_rowmask([0, 31, 32, 299], 300))
    for h in (sp_other, other, sp, index):
        h.close()


def test_masks_are_destroyed_alone_in_any_order_and_outlive_their_index():
    index, sp, rows, _ = build(1000, 37, 41)
    queries = make_queries(37)[:12]
    (q_off, q_terms), mm = csr(queries)
    want = [_native.pack_rowmask(tmo.match_rows(rows[0], rows[1], q, m), 1000) for q, m in queries]
    masks = index.match_masks(sp, q_off, q_terms, mm)
    for i in reversed(range(len(masks))):                 # reverse order; the survivors stay readable
        masks[i].close()
        assert all(np.array_equal(masks[j].words(), want[j]) for j in range(i))
    masks = index.match_masks(sp, q_off, q_terms, mm)
    order = np.random.default_rng(1).permutation(len(masks))
    for pos, i in enumerate(order):
        masks[i].close()
        for j in order[pos + 1:][:3]:
            assert np.array_equal(masks[j].words(), want[j])
    before = index.match_masks(sp, q_off, q_terms, mm)
    after = index.match_masks(sp, q_off, q_terms, mm)
    for m in before:
        m.close()
    sp.close(); index.close()                             # the masks keep no pointer into their index
    assert all(np.array_equal(m.words(), w) for m, w in zip(after, want))
    assert after[1].stats()["rows"] == int(sum(bin(int(x)).count("1") for x in want[1]))
    for m in after:
        m.close()


def _bits(outs):
    return [(o.cpu().numpy() if hasattr(o, "cpu") else o).tobytes() for o in outs]


def test_searches_take_a_produced_mask_like_a_listed_one():
    T = tile()
    n = T + 200
    index, sp, rows, _ = build(n, 37, 51)
    rng = np.random.default_rng(8)
    queries = [([3, 4], 1), ([5, 6], 1), ([1], 1), ([0, 1, 5], 2), ([2], 1), ([7, 8, 9, 10], 2)]
    nq = len(queries)
    (q_off, q_terms), mm = csr(queries)
    produced = index.match_masks(sp, q_off, q_terms, mm)
    listed = [index.rowmask(tmo.match_rows(rows[0], rows[1], q, m)) for q, m in queries]
    dense = rng.standard_normal((nq, DIM), dtype=np.float32)
    assert _bits(index.search_masked(dense, 10, produced)) == _bits(index.search_masked(dense, 10, listed))
    sq = sparse_text.csr_from_pairs([(np.asarray(q, np.uint32), np.full(len(q), 1.5, np.float32)) for q, _ in queries])
    assert _bits(index.search_sparse(sp, *sq, 10, masks=produced)) == _bits(index.search_sparse(sp, *sq, 10, masks=listed))
    fusion = index.fusion(nq * 2)
    hq = rng.standard_normal((nq, 2, DIM), dtype=np.float32)
    two = lambda ms: [m for m in ms for _ in range(2)]   # noqa: E731
    assert _bits(index.search_hybrid(hq, [10, 7], 8, fusion, masks=two(produced))) == _bits(index.search_hybrid(hq, [10, 7], 8, fusion, masks=two(listed)))
    grouping = index.grouping((np.arange(n) % 13).astype(np.int32), max_nq=64)
    a = index.search_sparse(sp, *sq, 4, masks=produced, grouping=grouping, group_size=2)
    b = index.search_sparse(sp, *sq, 4, masks=listed, grouping=grouping, group_size=2)
    assert _bits(a) == _bits(b)
    for h in produced + listed + [grouping, fusion, sp, index]:
        h.close()


# ---- the service ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def services(tmp_path_factory):
    mp = pytest.MonkeyPatch()
    mp.setenv("MILVUS_DB_PATH", str(tmp_path_factory.mktemp("db")))
    mp.setenv("MILVUS_COLLECTION_NAME", "icd10_text_match")
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


def test_service_routes_agree(services):
    ms, es, recs = services["ms"], services["es"], services["recs"]
    titles = [r["preferred_zh"] for r in recs]
    level = np.array([r.get("level", 1) for r in recs])
    words = ["结核", "伤寒", "霍乱", "感染", "zzzz", "肺结核", "其他", ""]
    texts = [titles[(7 * i) % len(titles)] for i in range(len(words))]
    exprs = [f'level >= 2 and TEXT_MATCH(preferred_zh, "{w}")' for w in words[:4]] + \
            [f'TEXT_MATCH(preferred_zh, "{w}", minimum_should_match=2) and level >= 2' for w in words[4:6]] + \
            [sparse_text.text_match_expr("preferred_zh", words[6], "all"), None]
    assert all(e is None or filter_expr.text_match_shape(e) is not None for e in exprs)
    vecs = np.asarray(es.encode_query_batch(texts), dtype=np.float32)
    device = ms.search_batch(vecs, 10, filter=exprs, filter_mode="mask")
    ms.TEXT_MATCH_ON_DEVICE = False
    try:
        host = ms.search_batch(vecs, 10, filter=exprs, filter_mode="mask")
        host_rows = [None if e is None else ms.filter_rows(e) for e in exprs]
    finally:
        ms.TEXT_MATCH_ON_DEVICE = True
    assert _bits(device) == _bits(host)
    # the host route's rows are the oracle's
    for e, w, rows in zip(exprs[:4], words[:4], host_rows[:4]):
        want = tmo.match_text(titles, sparse_text.analyze, w, 1)
        assert np.array_equal(rows, want[level[want] >= 2]), e
    assert len(host_rows[0]) > 0 and len(host_rows[4]) == 0
    # the two routes' bits, mask against mask
    index = ms._index
    cached = sorted(f["expression"] for f in ms.filter_masks())   # (the forced host route went through the mask cache; the device route adds nothing)
    made = ms._masks_for(index, exprs, len(exprs))
    for m, rows in zip(made, host_rows):
        if rows is None:
            assert m is None
        else:
            assert np.array_equal(m.words(), _native.pack_rowmask(rows, index.n))
    ms._release_masks(made)
    assert all(m is None or m.closed for m in made) and sorted(f["expression"] for f in ms.filter_masks()) == cached
    # the default mode (a view per expression) gives the same hits
    for q, e in enumerate(exprs):
        view = ms.search_batch(vecs[q:q + 1], 10, filter=e)
        assert [x[0].tobytes() for x in _bits_rows(view)] == [x[q].tobytes() for x in _bits_rows(device)], e
    # the other entries that take masks: one expression, device route against host route
    e = exprs[0]
    one = ms.search(vecs[0], 5, filter=e, filter_mode="mask")
    txt = ms.search_text(titles[3], 5, filter=e)
    ms.TEXT_MATCH_ON_DEVICE = False
    try:
        assert one == ms.search(vecs[0], 5, filter=e, filter_mode="mask") and one == ms.search(vecs[0], 5, filter=e)
        assert txt == ms.search_text(titles[3], 5, filter=e)
    finally:
        ms.TEXT_MATCH_ON_DEVICE = True
    assert one and all("结核" in h["title"] or "结" in h["title"] or "核" in h["title"] for h in one)


def _bits_rows(outs):
    return [(o.cpu().numpy() if hasattr(o, "cpu") else np.asarray(o)) for o in outs]


def test_a_refused_program_falls_back_to_one_match_masks_call(services):
    """FILTER_ON_DEVICE on, but S has 17 leaves and device_program refuses it: `S and TEXT_MATCH(...)` keeps section 17's call - the
    text parts of the whole batch in ONE match_masks call over S's host-made mask, no filter_masks call - and the masks are the
    host route's, word for word and in row count."""
    ms = services["ms"]
    index = ms._ready_index()
    S = " or ".join(f"level == {i}" for i in range(2, 19))
    exprs = [f'({S}) and TEXT_MATCH(preferred_zh, "{w}")' for w in ("结核", "伤寒", "霍乱 感染", "zzzz")]
    dev, cols = ms._device_columns(index)
    _sp, tx, field = ms._text_index()
    assert ms.FILTER_ON_DEVICE and ms.TEXT_MATCH_ON_DEVICE and dev is not None
    assert filter_expr.device_program(S, cols) is None
    assert all(filter_expr.device_program(e, cols, {field: tx}) is None and filter_expr.text_match_shape(e) is not None for e in exprs)
    assert 0 < len(ms.filter_rows(S)) < index.n   # (S does select: the text masks are built over a base mask)
    calls = {"match_masks": [], "filter_masks": []}
    real_match, real_filter = index.match_masks, index.filter_masks
    index.match_masks = lambda *a, **k: (calls["match_masks"].append(len(a[3])), real_match(*a, **k))[1]
    index.filter_masks = lambda *a, **k: (calls["filter_masks"].append(len(a[2]) - 1), real_filter(*a, **k))[1]
    try:
        made = ms._masks_for(index, exprs, len(exprs))
    finally:
        del index.match_masks, index.filter_masks
    assert calls == {"match_masks": [len(exprs)], "filter_masks": []}
    device = [(m.words(), m.stats()["rows"]) for m in made]
    assert all(getattr(m, "transient", False) for m in made)
    ms._release_masks(made)
    ms.TEXT_MATCH_ON_DEVICE = False
    try:
        host = [(m.words(), m.stats()["rows"]) for m in ms._masks_for(index, exprs, len(exprs))]
        rows = [ms.filter_rows(e) for e in exprs]
    finally:
        ms.TEXT_MATCH_ON_DEVICE = True
    for e, (dw, dr), (hw, hr), r in zip(exprs, device, host, rows):
        assert np.array_equal(dw, hw) and dr == hr == len(r), e
        assert np.array_equal(dw, _native.pack_rowmask(r, index.n)), e
    assert len(rows[0]) > 0 and len(rows[3]) == 0


def test_endpoints_take_a_text_match_filter(services):
    # (last of the module: the app's lifespan disconnects the installed services when the client closes)
    from fastapi.testclient import TestClient
    from rag_project_icd10_amd.api import app as appmod
    from rag_project_icd10_amd.services.multi_diagnosis_service import MultiDiagnosisService
    ms, es, recs = services["ms"], services["es"], services["recs"]
    expr = 'level >= 2 and TEXT_MATCH(preferred_zh, "伤寒")'
    allowed = {recs[i]["code"] for i in ms.filter_rows(expr)}
    assert allowed
    appmod.install_services(es, ms, MultiDiagnosisService(es, ms))
    try:
        with TestClient(appmod.app) as client:
            for mode in ("mask", "view"):
                r = client.post("/query", json={"text": "霍乱，伤寒；副伤寒", "top_k": 3, "filter": expr, "filter_mode": mode})
                body = r.json()
                assert r.status_code == 200 and body["candidates"], body
                assert all(c["code"] in allowed for m in body["diagnosis_matches"] for c in m["candidates"])
            h = client.post("/hybrid_query", json={"texts": ["伤寒", "副伤寒"], "top_k": 5, "req_limit": 20, "sparse": True, "filter": expr})
            assert h.status_code == 200, h.text
            assert h.json()["candidates"] and all(c["code"] in allowed for c in h.json()["candidates"])
            assert client.post("/query", json={"text": "霍乱", "filter": 'TEXT_MATCH(code, "x")'}).status_code == 400
            assert client.post("/query", json={"text": "霍乱", "filter": 'TEXT_MATCH(preferred_zh, "x", minimum_should_match=0)'}).status_code == 400
    finally:
        appmod.install_services(None, None, None)
