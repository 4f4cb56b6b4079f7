"""icd_rowmask_group_counts on the device against tests/facet_oracle.py: exact int32 arrays, no tolerance
anywhere. Row counts sit around a mask word (32 rows), a lane's 64 rows and the grid's segment (S rows); groupings around one group,
one group per row, sparse caller ids, a group across a segment boundary, a single row in the last partial word, and both sides of the
bound between the two accumulation forms (LDS histogram / global adds)."""
import ctypes

import numpy as np
import pytest

import facet_oracle as fo
from rag_project_icd10_amd import _native
from rag_project_icd10_amd.services import filter_expr as fe

pytestmark = pytest.mark.gpu

DIM = 32
S = _native.SELECT_SEGMENT_ROWS
LDS_G = _native.FACET_LDS_GROUPS
ROW_COUNTS = (1, 31, 32, 33, 64, 65, 257, S - 1, S, S + 1, 2 * S + 33)
R, NOT = 1, 6   # filter program words (include/icd_search.h ICD_FILTER_RANGE / _NOT)


def make_index(n, seed, max_nq=512, **kw):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, DIM), dtype=np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return _native.IcdIndex(x, rng.integers(1, 4, n).astype(np.int32), device=0, max_nq=max_nq, max_k=16, probe=False, **kw)


def mask_shapes(n, seed):
    """(name, bool [n] or None for a NULL entry)"""
    rng = np.random.default_rng(seed)
    rows = np.arange(n)
    return [
        ("empty", np.zeros(n, bool)), ("NULL", None), ("every row", np.ones(n, bool)), ("row 0", rows == 0), ("row n - 1", rows == n - 1),
        ("every other row", rows % 2 == 1), ("density 0.5", rng.random(n) < 0.5), ("density 1/1000", rng.random(n) < 1e-3),
    ]


def groupings_for(n, seed):
    """(name, caller ids int32 [n])"""
    rng = np.random.default_rng(seed)
    rows = np.arange(n)
    across = np.where(rows < S - 10, 4, np.where(rows < S + 10, 6, 9))          # group 6 holds the rows S - 10 .. S + 10: both sides of a segment's end
    last = rows % 4
    last[n - 1] = 77                                                            # a group of one row, the last of the last (partial) word
    return [
        ("G = 1", np.zeros(n, np.int64)), ("G = 2, alternating", rows % 2), ("G = n", rows[::-1].copy()),
        ("sparse ids", np.array([5, 1000, 7])[rng.integers(0, 3, n)]), ("across a segment", across), ("one row in the last word", last),
    ]


def to_host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def check(index, grouping, group_of, handles, bools, **kw):
    got = index.group_counts(handles, grouping, **kw)
    g = to_host(got)
    want = fo.counts_batch(bools, group_of)
    assert g.dtype == np.int32 and g.shape == want.shape, (g.dtype, g.shape, want.shape)
    bad = np.argwhere(g != want)
    assert bad.size == 0, f"n={index.n} G={want.shape[1]}: first differences at {bad[:4].tolist()}: {g[tuple(bad[0])]} vs {want[tuple(bad[0])]}"
    return got


def build_masks(index, shapes):
    handles = [None if m is None else index.rowmask(np.flatnonzero(m).astype(np.int64)) for _, m in shapes]
    return handles, [m for _, m in shapes]


@pytest.mark.parametrize("n", ROW_COUNTS)
def test_every_row_count_mask_and_grouping(n):
    index = make_index(n, 100 + n % 97)
    handles, bools = build_masks(index, mask_shapes(n, n))
    totals = index.count_rows(handles)
    for name, ids in groupings_for(n, n + 1):
        grouping = index.grouping(ids, max_nq=16)
        assert np.array_equal(grouping.group_ids, fo.dense(ids)[0]) and grouping.groups == len(grouping.group_ids), name
        host = check(index, grouping, ids, handles, bools)
        dev = check(index, grouping, ids, handles, bools, on_device=True)
        again = index.group_counts(handles, grouping)
        assert host.tobytes() == to_host(dev).tobytes() == again.tobytes(), (n, name)
        assert np.array_equal(host.sum(axis=1, dtype=np.int64), totals), (n, name)        # a row of counts sums to the mask's rows
        assert np.array_equal(host[1], np.bincount(fo.dense(ids)[1], minlength=grouping.groups)), (n, name)   # the NULL mask: the group sizes
        grouping.close()
    grouping = index.grouping(np.zeros(n, np.int32), max_nq=16)
    assert index.group_counts([], grouping).shape == (0, 1)   # nq = 0 does nothing
    grouping.close()
    index.close()


@pytest.fixture(scope="module")
def big():
    """n = 2 S + 33 with its mask shapes, shared by the tests of the bound and of the batches (nothing here is changed by a test)"""
    n = 2 * S + 33
    index = make_index(n, 7)
    handles, bools = build_masks(index, mask_shapes(n, 3))
    yield {"n": n, "index": index, "handles": handles, "bools": bools}
    index.close()


@pytest.mark.parametrize("G", (LDS_G - 1, LDS_G, LDS_G + 1))
@pytest.mark.parametrize("layout", ("scattered", "sorted"))
def test_both_accumulation_forms_and_their_edge(big, G, layout):
    n, index = big["n"], big["index"]
    rows = np.arange(n, dtype=np.int64)
    ids = rows * 7919 % G if layout == "scattered" else rows * G // n     # (7919 is coprime to all three: every group holds a row)
    grouping = index.grouping(ids, max_nq=16)
    assert grouping.groups == G
    host = check(index, grouping, ids, big["handles"], big["bools"])
    dev = check(index, grouping, ids, big["handles"], big["bools"], on_device=True)
    assert host.tobytes() == to_host(dev).tobytes() == index.group_counts(big["handles"], grouping).tobytes()
    assert np.array_equal(host.sum(axis=1, dtype=np.int64), index.count_rows(big["handles"]))
    grouping.close()


@pytest.mark.parametrize("nq", (1, 3, 300))
def test_batches_with_a_mask_of_their_own(big, nq):
    """300 host-output queries are two passes through the grouping's block (max_nq = 16: 256 queries a pass)"""
    n, index = big["n"], big["index"]
    rng = np.random.default_rng(nq)
    handles, bools = [], []
    for q in range(nq):
        m = None if q % 5 == 3 else rng.random(n) < (0.5, 0.03, 1e-3, 0.97)[q % 4]
        handles.append(None if m is None else index.rowmask(np.flatnonzero(m).astype(np.int64)))
        bools.append(m)
    rows = np.arange(n, dtype=np.int64)
    for ids in (rows * 2654435761 % 41, rows * 7919 % (LDS_G + 1)):
        grouping = index.grouping(ids, max_nq=16)
        a = check(index, grouping, ids, handles, bools)
        b = check(index, grouping, ids, handles, bools, on_device=True)
        assert a.tobytes() == to_host(b).tobytes()
        assert np.array_equal(a.sum(axis=1, dtype=np.int64), index.count_rows(handles))
        grouping.close()
    for h in handles:
        if h is not None:
            h.close()


def test_produced_masks_and_their_tail_bits():
    """masks filter_masks and match_masks made (bitsets inside one shared block), and a produced NOT at n = 33: whatever the buffer
    holds behind n, those bits count for no group. The oracle unpacks the masks' own words (icd_rowmask_read)."""
    for n in (33, S + 129):
        index = make_index(n, 17)
        cols = index.columns(np.ascontiguousarray(np.stack([np.arange(n), np.arange(n) % 3]).astype(np.int32)))
        progs = [[R, 0, 8, 8, NOT], [R, 1, 1, 2], [R, 1, 1, 2, NOT], [R, 0, n // 2, n], [R, 0, 8, 8]]
        rows = np.arange(n)
        want = [np.ones(n, bool), rows % 3 == 1, rows % 3 != 1, rows >= n // 2, np.zeros(n, bool)]
        off, words = fe.pack_programs([np.asarray(p, np.uint32) for p in progs])
        produced = index.filter_masks(cols, None, off, words)
        t0 = rows % 3 == 0   # term 0 in the rows 3 | r, term 1 in every row
        row_off = np.concatenate([[0], np.cumsum(1 + t0.astype(np.int64))])
        terms = np.concatenate([[0, 1] if t else [1] for t in t0]).astype(np.uint32)
        sp = index.sparse(row_off, terms, np.ones(len(terms), np.float32), 4, max_nq=64, max_k=16)
        produced += index.match_masks(sp, np.array([0, 1, 3, 4]), np.array([0, 0, 1, 1], np.uint32), np.array([1, 2, 1], np.int32))
        want += [t0, t0, np.ones(n, bool)]
        read = [m.words() for m in produced]
        for w, b in zip(read, want):   # (the masks are what they should be: the counts are checked on known rows)
            assert np.array_equal(fo.unpack(w, n), b)
        for name, ids in groupings_for(n, 5):
            grouping = index.grouping(ids, max_nq=16)
            got = check(index, grouping, ids, produced, want)
            assert np.array_equal(got, fo.counts_batch(read, ids, words=True)), name
            assert got[0].sum() == n == got[-1].sum() and np.array_equal(got.sum(axis=1, dtype=np.int64), index.count_rows(produced))
            grouping.close()
        for h in produced + [sp, cols]:
            h.close()
        index.close()


def raw(index, grouping, handles, out, nq=None, idx_handle=None, on_device=0, stream=None):
    """the C entry itself -> status; `out`: a numpy array or a torch CUDA tensor the caller filled"""
    nq = len(handles) if nq is None else nq
    table = (ctypes.c_void_p * max(len(handles), 1))(*handles)
    ptr = out.data_ptr() if hasattr(out, "data_ptr") else out.ctypes.data
    return index._lib.icd_rowmask_group_counts(index._h if idx_handle is None else idx_handle, grouping._h, ctypes.cast(table, ctypes.c_void_p), nq,
                                               ptr, on_device, stream)


def test_a_second_call_sees_nothing_of_the_first_and_repeats_are_the_same_bytes(big):
    import torch
    n, index = big["n"], big["index"]
    rows = np.arange(n, dtype=np.int64)
    first, second = [0, 2, 6, 1], [3, 7, 4, 5]   # (mask shapes; the second set counts fewer rows in most groups than the first)
    for ids in (rows * 2654435761 % 41, rows * 7919 % (LDS_G + 1)):
        grouping = index.grouping(ids, max_nq=16)
        G = grouping.groups
        wants = [fo.counts_batch([big["bools"][i] for i in pick], ids) for pick in (first, second)]
        dev = torch.full((4, G), -7, dtype=torch.int32, device="cuda")
        host = np.full((4, G), -7, np.int32)
        stream = _native._current_stream_ptr(0)
        for pick, want in list(zip((first, second), wants)) + [(second, wants[1])]:
            table = [None if big["handles"][i] is None else big["handles"][i]._h.value for i in pick]
            assert raw(index, grouping, table, dev, on_device=1, stream=stream) == 0
            assert raw(index, grouping, table, host) == 0
            torch.cuda.synchronize()
            assert np.array_equal(dev.cpu().numpy(), want) and host.tobytes() == want.tobytes()
        grouping.close()


def test_refusals_leave_the_output_the_index_and_the_grouping_alone():
    INVALID, UNSUPPORTED, STATE = -1, -4, -5
    n = 300
    index, other = make_index(n, 1, max_nq=8), make_index(n, 2, max_nq=8)
    some = np.arange(0, n, 3, dtype=np.int64)
    bools = [np.isin(np.arange(n), some), None]
    ids = np.arange(n) % 7
    mask, foreign, dead = index.rowmask(some), other.rowmask(some), index.rowmask(some)
    dead.close()   # (refused through the binding below: the C entry must not be handed a freed handle)
    view = index.view(np.arange(0, n, 2, dtype=np.int64))
    grouping, theirs, on_view = index.grouping(ids), other.grouping(ids), view.grouping(ids[::2])
    gone = index.grouping(ids)
    gone.close()
    good = [mask._h.value, None]

    def fine():
        check(index, grouping, ids, [mask, None], bools)

    fine()
    cases = [
        ("a grouping of another index", dict(grouping=theirs, handles=good), INVALID),
        ("a grouping of a view", dict(grouping=on_view, handles=good), UNSUPPORTED),
        ("a view as idx", dict(grouping=on_view, handles=[None, None], idx_handle=view._h), UNSUPPORTED),
        ("a view as idx, the parent's grouping", dict(grouping=grouping, handles=[None, None], idx_handle=view._h), UNSUPPORTED),
        ("nq above max_nq", dict(grouping=grouping, handles=[None] * 9), INVALID),
        ("a mask of another index", dict(grouping=grouping, handles=[mask._h.value, foreign._h.value]), INVALID),
        ("nq below 0", dict(grouping=grouping, handles=good, nq=-1), INVALID),
        ("no index", dict(grouping=grouping, handles=good, idx_handle=ctypes.c_void_p()), STATE),
    ]
    for name, kw, want in cases:
        out = np.full((9, 7), -7, np.int32)
        rc = raw(index, out=out, **kw)
        assert rc == want, (name, rc, index._lib.icd_last_error())
        assert (out == -7).all(), name   # no side effect on the output
        fine()
    # the binding: ValueError for what the library calls invalid, IcdError for a closed partner or a view
    for kw in (dict(masks=[mask, foreign], grouping=grouping), dict(masks=[None] * 9, grouping=grouping), dict(masks=[mask], grouping=theirs)):
        with pytest.raises(ValueError):
            index.group_counts(**kw)
        fine()
    for who, kw, code in ((index, dict(masks=[dead], grouping=grouping), STATE), (index, dict(masks=[mask], grouping=gone), STATE),
                          (view, dict(masks=[None], grouping=on_view), UNSUPPORTED), (index, dict(masks=[mask], grouping=on_view), UNSUPPORTED)):
        with pytest.raises(_native.IcdError) as e:
            who.group_counts(**kw)
        assert e.value.code == code
        fine()
    # the grouping still searches after all of it
    q = np.random.default_rng(3).standard_normal((2, DIM), dtype=np.float32)
    assert index.search_grouped(q, 3, 2, grouping, reweighted=False)[1].shape == (2, 6)
    fine()
    for h in (mask, foreign, grouping, theirs, on_view, view, other, index):
        h.close()
