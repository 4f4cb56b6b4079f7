"""icd_rowmask_select on the device against tests/mask_select_oracle.py, byte for byte: ids, total and taken
of every query of a batch. Integer output: no tolerance anywhere. Row counts sit around a mask word (32 rows), a mask tile (128) and
the select's segment (S rows); offsets at both ends of a word, of a segment's ranks and of the mask's total."""
import ctypes

import numpy as np
import pytest

import mask_select_oracle as mso
from rag_project_icd10_amd import _native
from rag_project_icd10_amd.services import filter_expr as fe

pytestmark = pytest.mark.gpu

DIM = 32
S = _native.SELECT_SEGMENT_ROWS
LIMITS = (1, 7, 64, 16384)
ROW_COUNTS = (1, 31, 32, 33, 127, 128, 129, 257, S - 1, S, S + 1, 2 * S + 33)
R, NOT = 1, 6   # filter program words (include/icd_search.h ICD_FILTER_RANGE / _NOT)


def make_index(n, seed, max_nq=512, **kw):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, DIM), dtype=np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return _native.IcdIndex(x, rng.integers(1, 4, n).astype(np.int32), device=0, max_nq=max_nq, max_k=16, probe=False, **kw)


def mask_shapes(n, seed):
    """(name, bool [n] or None for a NULL entry, build as a mask even when every row is set)"""
    rng = np.random.default_rng(seed)
    rows = np.arange(n)
    return [
        ("empty", np.zeros(n, bool)), ("NULL", None), ("every row", np.ones(n, bool)), ("row 0", rows == 0), ("row n - 1", rows == n - 1),
        ("every other row", rows % 2 == 1), ("one row per segment", rows % S == min(S, n) // 2),
        ("density 0.5", rng.random(n) < 0.5), ("density 1/1000", rng.random(n) < 1e-3),
    ]


def offsets_for(mask, n):
    """0; inside a word; exactly at a segment's base rank and one before it; total - 1, total, total + 5"""
    full = np.ones(n, bool) if mask is None else mask
    total = int(full.sum())
    base = int(full[:S].sum()) if n > S else total // 2   # the rank of the second segment's first set row
    return [max(o, 0) for o in (0, 5, base, base - 1, total - 1, total, total + 5)]


def as_bytes(outs):
    return [(o.cpu().numpy() if hasattr(o, "cpu") else np.asarray(o)).tobytes() for o in outs]


def check(index, handles, bools, offsets, limit, **kw):
    got = index.select_rows(handles, limit, offsets, **kw)
    want = mso.select_batch(bools, index.n, offsets, limit)
    host = [o.cpu().numpy() if hasattr(o, "cpu") else o for o in got]
    for g, w, name in zip(host, want, ("ids", "total", "taken")):
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, g.shape)
        bad = np.argwhere(g != w)
        assert bad.size == 0, f"n={index.n} limit={limit} {name}: first differences at {bad[:4].tolist()}: {g[tuple(bad[0])]} vs {w[tuple(bad[0])]}"
    return got


@pytest.mark.parametrize("n", ROW_COUNTS)
def test_every_shape_offset_and_limit(n):
    index = make_index(n, 100 + n % 97)
    shapes = mask_shapes(n, n)
    handles, bools, offsets = [], [], []
    for name, m in shapes:
        h = None if m is None else index.rowmask(np.flatnonzero(m).astype(np.int64))
        for o in offsets_for(m, n):
            handles.append(h); bools.append(m); offsets.append(o)
    assert len(handles) == 63
    for limit in LIMITS:   # (16384 x 63 ids exceed the host staging of max_nq = 512: that call goes through device outputs)
        first = check(index, handles, bools, offsets, limit)
        again = index.select_rows(handles, limit, offsets)
        dev = index.select_rows(handles, limit, offsets, on_device=True)
        assert as_bytes(first) == as_bytes(again) == as_bytes(dev), (n, limit)
    # offsets=None and one offset for every query
    check(index, handles[::7], bools[::7], None, 7)
    got = index.select_rows(handles[::7], 7, 3)
    assert as_bytes(got) == as_bytes(mso.select_batch(bools[::7], n, [3] * 9, 7))
    # the count alone
    assert np.array_equal(index.count_rows(handles[::7]), mso.select_batch(bools[::7], n, None, 1)[1])
    index.close()


@pytest.mark.parametrize("nq", (1, 3, 300))
def test_batches_with_a_mask_and_an_offset_of_their_own(nq):
    n = 2 * S + 33
    index = make_index(n, 7)
    rng = np.random.default_rng(nq)
    handles, bools, offsets = [], [], []
    for q in range(nq):
        if q % 5 == 3:
            m = None
        else:
            m = rng.random(n) < (0.5, 0.03, 1e-3, 0.97)[q % 4]
        handles.append(None if m is None else index.rowmask(np.flatnonzero(m).astype(np.int64)))
        bools.append(m)
        total = n if m is None else int(m.sum())
        offsets.append(int(rng.integers(0, total + 3)))
    for limit in (7, 64):
        a = check(index, handles, bools, offsets, limit)
        b = check(index, handles, bools, offsets, limit, on_device=True)
        assert as_bytes(a) == as_bytes(b)
    check(index, handles[:3], bools[:3], offsets[:3], 16384)
    assert index.select_rows([], 5)[0].shape == (0, 5)   # nq = 0 does nothing
    index.close()


def test_produced_masks_and_their_tail_bits():
    """masks filter_masks and match_masks made (bitsets inside one shared block), and a produced NOT at n = 33: the kernel that made
    it cleared the bits behind n, the select clears them again whatever the buffer holds"""
    for n in (33, S + 129):
        index = make_index(n, 17)
        cols = index.columns(np.ascontiguousarray(np.stack([np.arange(n), np.arange(n) % 3]).astype(np.int32)))
        progs = [[R, 0, 8, 8, NOT], [R, 1, 1, 2], [R, 1, 1, 2, NOT], [R, 0, n // 2, n], [R, 0, 8, 8]]
        rows = np.arange(n)
        want = [np.ones(n, bool), rows % 3 == 1, rows % 3 != 1, rows >= n // 2, np.zeros(n, bool)]
        off, words = fe.pack_programs([np.asarray(p, np.uint32) for p in progs])
        produced = index.filter_masks(cols, None, off, words)
        # term 0 in the rows 3 | r, term 1 in every row
        t0 = rows % 3 == 0
        row_off = np.concatenate([[0], np.cumsum(1 + t0.astype(np.int64))])
        terms = np.concatenate([[0, 1] if t else [1] for t in t0]).astype(np.uint32)
        sp = index.sparse(row_off, terms, np.ones(len(terms), np.float32), 4, max_nq=64, max_k=16)
        matched = index.match_masks(sp, np.array([0, 1, 3, 4]), np.array([0, 0, 1, 1], np.uint32), np.array([1, 2, 1], np.int32))
        produced += matched
        want += [t0, t0, np.ones(n, bool)]
        for m, w in zip(produced, want):   # (the masks are what they should be: the select is checked on known rows)
            assert np.array_equal(np.unpackbits(m.words().view(np.uint8), bitorder="little")[:n].astype(bool), w)
        for limit in (7, 16384):
            for offset in (0, 2, n // 3):
                ids, total, taken = check(index, produced, want, [offset] * len(produced), limit)
                assert ids.max() < n and total[0] == n and taken[0] == min(n - offset, limit)
        for h in produced + [sp, cols]:
            h.close()
        index.close()


def raw(index, handles, limit, offsets=None, nq=None, idx_handle=None, outs="host", stream=None):
    """the C entry itself -> (status, ids, total, taken); outputs pre-filled with a pattern"""
    nq = len(handles) if nq is None else nq
    table = (ctypes.c_void_p * max(len(handles), 1))(*handles)
    ids = np.full((max(nq, 1), max(limit, 1)), -7, np.int64)
    total, taken = np.full(max(nq, 1), -7, np.int64), np.full(max(nq, 1), -7, np.int32)
    off = None if offsets is None else np.asarray(offsets, np.int64)
    rc = index._lib.icd_rowmask_select(index._h if idx_handle is None else idx_handle, ctypes.cast(table, ctypes.c_void_p), nq,
                                       None if off is None else off.ctypes.data, limit, ids.ctypes.data, total.ctypes.data, taken.ctypes.data,
                                       0, stream)
    return rc, ids, total, taken


def test_refusals_leave_the_outputs_and_the_index_alone():
    import torch
    INVALID, UNSUPPORTED, STATE = -1, -4, -5
    n = 300
    index, other = make_index(n, 1, max_nq=8), make_index(n, 2, max_nq=8)
    some = np.arange(0, n, 3, dtype=np.int64)
    bools = [np.isin(np.arange(n), some), None]
    mask, foreign, dead = index.rowmask(some), other.rowmask(some), index.rowmask(some)
    dead.close()   # (refused through the binding below: the C entry must not be handed a freed handle)
    view = index.view(np.arange(0, n, 2, dtype=np.int64))
    good = [mask._h.value, None]

    def fine():
        check(index, [mask, None], bools, [4, 290], 16)

    fine()
    cases = [
        ("a mask of another index", dict(handles=[mask._h.value, foreign._h.value], limit=4), INVALID),
        ("a view", dict(handles=[None, None], limit=4, idx_handle=view._h), UNSUPPORTED),
        ("limit 0", dict(handles=good, limit=0), INVALID),
        ("limit 16385", dict(handles=good, limit=16385), INVALID),
        ("a negative offset", dict(handles=good, limit=4, offsets=[0, -1]), INVALID),
        ("nq above max_nq", dict(handles=[None] * 9, limit=4), INVALID),
        ("nq below 0", dict(handles=good, limit=4, nq=-1), INVALID),
        ("no index", dict(handles=good, limit=4, idx_handle=ctypes.c_void_p()), STATE),
    ]
    for name, kw, want in cases:
        rc, ids, total, taken = raw(index, **kw)
        assert rc == want, (name, rc, index._lib.icd_last_error())
        assert (ids == -7).all() and (total == -7).all() and (taken == -7).all(), name   # no side effect on the outputs
        fine()
    lib = index._lib
    assert lib.icd_rowmask_select(index._h, None, 2, None, 4, None, None, None, 0, None) == INVALID   # no out_total, no table
    # the binding: ValueError for what the library calls invalid, IcdError for a closed partner or a view
    for kw in (dict(masks=[mask, foreign], limit=4), dict(masks=[mask], limit=0), dict(masks=[mask], limit=16385),
               dict(masks=[mask, None], limit=4, offsets=[0, -1]), dict(masks=[None] * 9, limit=4), dict(masks=[mask, None], limit=4, offsets=[1, 2, 3])):
        with pytest.raises(ValueError):
            index.select_rows(**kw)
        fine()
    with pytest.raises(_native.IcdError) as e:
        index.select_rows([dead], 4)
    assert e.value.code == STATE
    with pytest.raises(_native.IcdError) as e:
        view.select_rows([None], 4)
    assert e.value.code == UNSUPPORTED
    fine()
    # a capturing stream: refused, the capture survives and ends with a search that may be captured
    dq = torch.from_numpy(np.random.default_rng(3).standard_normal((2, DIM), dtype=np.float32)).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        index.search_reweighted(dq, 5)   # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        rc, ids, total, taken = raw(index, good, 4, stream=_native._current_stream_ptr(0))
        said = lib.icd_last_error().decode()
        ok = index.search_reweighted(dq, 5)
    graph.replay()
    torch.cuda.synchronize()
    assert rc == INVALID and "captured" in said and (ids == -7).all() and (total == -7).all()
    assert as_bytes(ok) == as_bytes(index.search_reweighted(dq.cpu().numpy(), 5))
    fine()
    for h in (mask, foreign, view, other, index):
        h.close()
