"""The contract every search entry point of libicdsearch shares (run with -m gpu on an MI355X): plain, reweighted, range, masked,
grouped and hybrid searches give a host caller the bytes they give a device caller whatever staging the call takes (the one-query
path, the pinned block, the staged copies, several query blocks / host pieces); every family refuses the same bad arguments with
the same codes, inside a stream capture too, and leaves the index as it was; a grouping does not outlive its index's identity.
Nothing here knows how the library arranges those checks: the tests go through IcdIndex and, where the wrapper would answer first,
through the C entry points."""
import ctypes as C

import numpy as np
import pytest

from conftest import icd_levels, unit_rows

pytestmark = pytest.mark.gpu

from rag_project_icd10_amd import _native  # noqa: E402
from rag_project_icd10_amd._native import MODE_AUTO, MODE_EXACT, IcdIndex  # noqa: E402

N, DIM, NQ = 384, 64, 600          # three 128-row tiles
_S = {}


def _setup():
    if not _S:
        corpus, levels = unit_rows(N, DIM, 311), icd_levels(N, 312)
        index = IcdIndex(corpus, levels, max_nq=600, max_k=128)
        other = IcdIndex(corpus, levels, max_nq=600, max_k=128)
        rows = np.sort(np.random.default_rng(313).choice(N, 100, replace=False)).astype(np.int64)
        half = np.arange(0, N, 2, dtype=np.int64)
        group_of = (np.arange(N) * 2654435761 % 23).astype(np.int32)
        _S.update(corpus=corpus, levels=levels, q=unit_rows(NQ, DIM, 314), index=index, other=other, view=index.view(rows),
                  mask=index.rowmask(half), other_mask=other.rowmask(half), grouping=index.grouping(group_of, max_nq=520),
                  fusion=index.fusion(600), group_of=group_of)
    return _S


def _bits(outs):
    return [np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a).tobytes() for a in outs]


def _both(call, *arrays):
    """call(*arrays) with numpy arguments and with the same arguments as CUDA tensors: every output, byte for byte"""
    import torch
    host = call(*arrays)
    dev = call(*[None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays])
    torch.cuda.synchronize()
    assert all(not hasattr(a, "cpu") for a in host) and all(a.is_cuda for a in dev)
    assert len(host) == len(dev) and _bits(host) == _bits(dev)
    return host


# ---- a. staging equivalence --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq,k", [(1, 5), (3, 5), (40, 100)])   # the one-query path; pinned outputs; 4 000 slots > the pinned block's 2 730
def test_host_and_device_callers_get_the_same_bytes(nq, k):
    s = _setup()
    index, q = s["index"], s["q"][:nq]
    raw, _ids = index.search(q, 128)
    lo, hi = raw[:, 60].copy(), raw[:, 3].copy()                  # a band per query: ranks 3 .. 59 of its ranking
    cursor = (raw[:, 10].copy(), _ids[:, 10].copy())
    for mode in (MODE_AUTO, MODE_EXACT):
        _both(lambda x: index.search(x, k, mode), q)
        _both(lambda x: index.search_reweighted(x, k, mode), q)
    for rw in (True, False):
        got = _both(lambda x, a, b: index.search_range(x, k, radius=a, range_filter=b, reweighted=rw), q, lo, hi)
        assert (got[-2][:, 0] >= 0).all()                          # (the band is not empty: the comparison is over hits, not padding)
        _both(lambda x, a, b: index.search_range(x, k, after=(a, b), reweighted=rw), q, *cursor)
        _both(lambda x, a: index.search_masked(x, k, s["mask"], radius=a, reweighted=rw), q, lo)
        _both(lambda x: index.search_masked(x, k, [s["mask"] if i % 2 else None for i in range(nq)], reweighted=rw), q)
        gk, gs = (k, 1) if k > 64 else (k, 2)
        _both(lambda x: index.search_grouped(x, gk, gs, s["grouping"], reweighted=rw), q)
        q3 = np.ascontiguousarray(np.stack([q, s["q"][100:100 + nq]], axis=1))
        _both(lambda x: index.search_hybrid(x, (5, 3), k, s["fusion"], reweighted=rw), q3)
        _both(lambda x, a: index.search_hybrid(x, (5, 3), k, s["fusion"], ranker="weighted", weights=[1.0, 0.5], norm="atan",
                                               masks=[[s["mask"], None]] * nq, radius=a, reweighted=rw),
              q3, np.ascontiguousarray(np.stack([lo, lo], axis=1)))


def test_several_query_blocks_and_host_pieces():
    s = _setup()
    index = s["index"]
    for rw in (True, False):
        _both(lambda x: index.search_grouped(x, 2, 2, s["grouping"], reweighted=rw), s["q"][:513])   # two 512-query blocks
    q3 = np.ascontiguousarray(s["q"][:514].reshape(257, 2, DIM))                                      # two 256-query host pieces
    _both(lambda x: index.search_hybrid(x, (5, 3), 5, s["fusion"], mode=MODE_AUTO), q3)
    masks = [[None, None] for _ in range(257)]
    masks[256][1] = s["mask"]
    radius = np.full((257, 2), -np.inf, np.float32)
    radius[3, 0] = 0.05
    got = _both(lambda x, a: index.search_hybrid(x, (5, 3), 5, s["fusion"], mode=MODE_AUTO, masks=masks, radius=a), q3, radius)
    assert (got[2][:, 0] >= 0).all()


# ---- b. the error table ------------------------------------------------------------------------------------------------------
class _Calls:
    """The six entry families through the C ABI with host buffers; every keyword replaces one argument."""

    def __init__(self, s):
        self.s, self.lib = s, s["index"]._lib
        self.q = np.ascontiguousarray(np.concatenate([s["q"], s["q"][:8]]))                 # 608 rows: nq = 601 stays inside it
        n = 608 * 128
        self.adj, self.fused, self.raw = np.zeros(n), np.zeros(n), np.zeros(n, np.float32)
        self.ids, self.lv, self.grp, self.bits = np.zeros(n, np.int64), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.uint32)
        self.junk = np.zeros(64, np.uint8)                                                   # a handle that is no row mask

    @staticmethod
    def p(a):
        return None if a is None else (a if isinstance(a, int) else (a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data))

    def table(self, masks, nq):
        """masks: one IcdRowMask / raw pointer per query (None entries allowed) -> the uint64 table the C entry points take"""
        if masks is None:
            return None
        masks = list(masks) if isinstance(masks, (list, tuple)) else [masks] * max(nq, 1)
        return np.array([0 if m is None else (m if isinstance(m, int) else m._h.value) for m in masks], np.uint64)

    def plain(self, index=None, nq=2, k=5, q=None, out=None, ids=None, dev=0, stream=None, mode=MODE_AUTO):
        h = (index or self.s["index"])._h
        return self.lib.icd_index_search(h, self.p(self.q if q is None else q), nq, k, dev, mode, self.p(self.raw if out is None else out),
                                         self.p(self.ids if ids is None else ids), dev, stream)

    def reweighted(self, index=None, nq=2, k=5, q=None, adj="own", dev=0, stream=None):
        h = (index or self.s["index"])._h
        return self.lib.icd_index_search_reweighted(h, self.p(self.q if q is None else q), nq, k, dev, MODE_AUTO,
                                                    self.p(self.adj if isinstance(adj, str) else adj), self.p(self.raw), self.p(self.ids),
                                                    self.p(self.lv), dev, stream)

    def band(self, index=None, masks=None, nq=2, k=5, q=None, radius=None, range_filter=None, a_s=None, a_i=None, raw="own", qdev=0,
             bdev=0, odev=0, outs=None, stream=None):
        """icd_index_search_range (masks None) or icd_index_search_masked"""
        h = (index or self.s["index"])._h
        adj, raw_, ids, lv = outs or (self.adj, self.raw if isinstance(raw, str) else raw, self.ids, self.lv)
        tail = (self.p(self.q if q is None else q), nq, k, qdev, self.p(radius), self.p(range_filter), self.p(a_s), self.p(a_i), bdev, 1,
                self.p(adj), self.p(raw_), self.p(ids), self.p(lv), odev, stream)
        if masks is None:
            return self.lib.icd_index_search_range(h, *tail)
        self.keep = self.table(masks, nq)
        return self.lib.icd_index_search_masked(h, self.keep.ctypes.data, *tail)

    def grouped(self, index=None, grouping=None, nq=2, k=2, gs=2, q=None, ids="own", dev=0, outs=None, stream=None):
        h = (index or self.s["index"])._h
        adj, raw, ids_, lv, grp = outs or (self.adj, self.raw, self.ids if isinstance(ids, str) else ids, self.lv, self.grp)
        return self.lib.icd_index_search_grouped(h, (grouping or self.s["grouping"])._h, self.p(self.q if q is None else q), nq, k, gs, dev, 1,
                                                 self.p(adj), self.p(raw), self.p(ids_), self.p(lv), self.p(grp), dev, stream)

    def hybrid(self, index=None, fusion=None, nq=2, R=2, limits=(5, 3), masks=None, radius=None, range_filter=None, ranker=0, weights=None,
               norm=0, k=5, q=None, fused="own", qdev=0, bdev=0, odev=0, outs=None, stream=None):
        h = (index or self.s["index"])._h
        lim = np.array(list(limits) + [1] * 8, np.int32)
        w = None if weights is None else np.array(list(weights) + [0.0] * 8, np.float64)
        self.keep = self.table(masks, nq * R)
        adj, fused_, ids, lv, bits = outs or (self.adj, self.fused if isinstance(fused, str) else fused, self.ids, self.lv, self.bits)
        return self.lib.icd_index_search_hybrid(h, (fusion or self.s["fusion"])._h, self.p(self.q if q is None else q), nq, R, qdev,
                                                lim.ctypes.data, self.p(self.keep), self.p(radius), self.p(range_filter), bdev, MODE_AUTO, ranker,
                                                60.0, self.p(w), norm, k, 1, self.p(adj), self.p(fused_), self.p(ids), self.p(lv), self.p(bits),
                                                odev, stream)


def test_every_family_refuses_the_same_arguments_with_the_same_codes():
    import torch
    s = _setup()
    index, other, view, mask, q = s["index"], s["other"], s["view"], s["mask"], s["q"]
    c = _Calls(s)
    f32 = lambda *v: np.array(v, np.float32)
    before = _bits(index.search_reweighted(q[:40], 10)) + _bits(index.search_masked(q[:40], 10, mask))
    other_grouping, other_fusion, view_fusion = other.grouping(s["group_of"], max_nq=8), other.fusion(16), view.fusion(16)
    closed = index.rowmask(np.arange(10))
    closed.close()
    junk = c.junk.ctypes.data
    nan, inv, four = f32(0.1, np.nan), (f32(0.1, 0.5), f32(0.2, 0.5)), f32(0.1, 0.1, 0.1, 0.1)
    gone = (_native.IcdError, -5)   # (a wrapper row: the code travels in the exception)
    table = [
        # NaN radius; radius >= range_filter; a cursor with a score but no ids
        (lambda: c.band(radius=nan), -1), (lambda: c.band(masks=mask, radius=nan), -1),
        (lambda: c.hybrid(radius=f32(0.1, 0.1, np.nan, 0.1)), -1), (lambda: c.hybrid(masks=mask, radius=f32(0.1, 0.1, np.nan, 0.1)), -1),
        (lambda: c.band(radius=inv[0], range_filter=inv[1]), -1), (lambda: c.band(masks=mask, radius=inv[0], range_filter=inv[1]), -1),
        (lambda: c.hybrid(radius=four, range_filter=f32(0.2, 0.2, 0.2, 0.1)), -1),
        (lambda: c.band(a_s=f32(1, 1)), -1), (lambda: c.band(masks=mask, a_s=f32(1, 1)), -1),
        (lambda: c.band(a_i=np.zeros(2, np.int64)), -1), (lambda: c.band(masks=mask, a_i=np.zeros(2, np.int64)), -1),
        # k = 0 and k = 129
        (lambda: c.plain(k=0), -1), (lambda: c.plain(k=129), -1), (lambda: c.reweighted(k=0), -1), (lambda: c.reweighted(k=129), -1),
        (lambda: c.band(k=0), -1), (lambda: c.band(k=129), -1), (lambda: c.band(masks=mask, k=0), -1), (lambda: c.band(masks=mask, k=129), -1),
        (lambda: c.grouped(k=0), -1), (lambda: c.grouped(k=129, gs=1), -1), (lambda: c.grouped(k=2, gs=0), -1), (lambda: c.grouped(k=65, gs=2), -1),
        (lambda: c.hybrid(k=0), -1), (lambda: c.hybrid(k=129), -1),
        (lambda: index.search(q[:2], 0), ValueError), (lambda: index.search_reweighted(q[:2], 129), ValueError),
        (lambda: index.search_range(q[:2], 0), ValueError), (lambda: index.search_masked(q[:2], 129, mask), ValueError),
        (lambda: index.search_grouped(q[:2], 65, 2, s["grouping"]), ValueError),
        # a NULL required output
        (lambda: c.plain(out=0), -1), (lambda: c.plain(ids=0), -1), (lambda: c.reweighted(adj=None), -1), (lambda: c.band(raw=None), -1),
        (lambda: c.band(masks=mask, raw=None), -1), (lambda: c.grouped(ids=None), -1), (lambda: c.hybrid(fused=None), -1),
        # nq above the limit
        (lambda: c.plain(nq=601), -1), (lambda: c.reweighted(nq=601), -1), (lambda: c.band(nq=601), -1),
        (lambda: c.band(masks=mask, nq=601), -1), (lambda: c.grouped(nq=521), -1), (lambda: c.hybrid(nq=601, R=1), -1),
        (lambda: c.hybrid(nq=301, R=2), -1),
        # a handle that is no mask; a closed mask (the wrapper's answer: the handle is gone)
        (lambda: c.band(masks=[mask, junk]), -5), (lambda: c.hybrid(masks=[None, mask, junk, None]), -5),
        (lambda: index.search_masked(q[:2], 5, closed), gone), (lambda: index.search_masked(q[:2], 5, [mask, closed]), gone),
        (lambda: index.search_hybrid(q[:4].reshape(2, 2, DIM), (5, 3), 5, s["fusion"], masks=[None, closed, None, None]), gone),
        # a mask, grouping or fusion of the other index
        (lambda: c.band(masks=s["other_mask"]), -1), (lambda: c.band(masks=[mask, s["other_mask"]]), -1),
        (lambda: c.hybrid(masks=[None, None, None, s["other_mask"]]), -1), (lambda: c.grouped(grouping=other_grouping), -1),
        (lambda: c.hybrid(fusion=other_fusion), -1), (lambda: c.band(index=other, masks=mask), -1),
        # any mask on the view
        (lambda: c.band(index=view, masks=mask), -4), (lambda: c.band(index=view, masks=[None, None]), -4),
        (lambda: c.hybrid(index=view, fusion=view_fusion, masks=mask), -4),
        (lambda: c.hybrid(index=view, fusion=view_fusion, masks=[None, None, None, None]), -4),
        # hybrid's own
        (lambda: c.hybrid(R=0), -1), (lambda: c.hybrid(R=9), -1), (lambda: c.hybrid(limits=(5, 0)), -1), (lambda: c.hybrid(limits=(129, 3)), -1),
        (lambda: c.hybrid(ranker=1, weights=(1.5, 0.5)), -1), (lambda: c.hybrid(ranker=1, weights=(np.nan, 0.5)), -1),
        (lambda: c.hybrid(ranker=1, weights=None), -1), (lambda: c.hybrid(ranker=7), -1), (lambda: c.hybrid(ranker=1, weights=(1.0, 0.5), norm=9), -1),
        (lambda: index.search_hybrid(q[:4].reshape(2, 2, DIM), (5, 3), 5, s["fusion"], ranker="borda"), ValueError),
        (lambda: index.search_hybrid(q[:4].reshape(2, 2, DIM), (5, 3), 5, s["fusion"], ranker="weighted", weights=[1.0, 0.5], norm="l2"), ValueError),
        (lambda: index.search_masked(q[:4], 5, [mask] * 3), ValueError),
    ]
    for row, (call, want) in enumerate(table):
        if isinstance(want, tuple):
            with pytest.raises(want[0]) as e:
                call()
            assert e.value.code == want[1], row
        elif isinstance(want, int):
            rc = call()
            assert rc == want, (row, rc, c.lib.icd_last_error().decode())
        else:
            with pytest.raises(want):
                call()
    assert "another index" in (c.band(masks=s["other_mask"]), c.lib.icd_last_error().decode())[1]
    assert "another index" in (c.grouped(grouping=other_grouping), c.lib.icd_last_error().decode())[1]
    assert "another index" in (c.hybrid(fusion=other_fusion), c.lib.icd_last_error().decode())[1]
    assert "a masked search returns 1 .. 128" in (c.band(masks=mask, k=0), c.lib.icd_last_error().decode())[1]
    assert "a range search returns 1 .. 128" in (c.band(k=0), c.lib.icd_last_error().decode())[1]

    # the same calls while a stream capture is active: whatever would synchronise or stage on the host is refused, the capture
    # survives and ends cleanly with the one search that may be captured
    dq, dq3 = torch.from_numpy(q[:2]).cuda(), torch.from_numpy(np.ascontiguousarray(q[:4])).cuda()
    mk = lambda dt: torch.empty((2, 128), dtype=dt, device="cuda")
    d_adj, d_fused, d_raw, d_ids, d_lv, d_grp, d_bits = (mk(torch.float64), mk(torch.float64), mk(torch.float32), mk(torch.int64),
                                                         mk(torch.int32), mk(torch.int32), mk(torch.int32))
    d_lo = torch.full((4,), 0.01, dtype=torch.float32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        index.search_reweighted(dq, 5)   # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        st = _native._current_stream_ptr(0)
        band_outs, grp_outs, hy_outs = (d_adj, d_raw, d_ids, d_lv), (d_adj, d_raw, d_ids, d_lv, d_grp), (d_adj, d_fused, d_ids, d_lv, d_bits)
        captured = [
            # host buffers
            lambda: c.plain(stream=st), lambda: c.reweighted(stream=st), lambda: c.band(stream=st), lambda: c.band(masks=mask, stream=st),
            lambda: c.grouped(stream=st), lambda: c.hybrid(stream=st),
            # device buffers, host bounds
            lambda: c.band(q=dq, qdev=1, odev=1, outs=band_outs, radius=f32(0.01, 0.01), stream=st),
            lambda: c.hybrid(q=dq3, qdev=1, odev=1, outs=hy_outs, radius=four, stream=st),
            # device buffers and bounds, a mask table
            lambda: c.band(q=dq, qdev=1, odev=1, bdev=1, outs=band_outs, masks=mask, radius=d_lo, stream=st),
            lambda: c.band(q=dq, qdev=1, odev=1, bdev=1, outs=band_outs, masks=mask, stream=st),
            lambda: c.hybrid(q=dq3, qdev=1, odev=1, bdev=1, outs=hy_outs, masks=mask, stream=st),
        ]
        codes = [(call(), "captured" in c.lib.icd_last_error().decode()) for call in captured]   # (each refusal is the capture's)
        ok = index.search_reweighted(dq, 5)
        okg = c.grouped(q=dq, dev=1, outs=grp_outs, stream=st)
    graph.replay()
    torch.cuda.synchronize()
    assert codes == [(-1, True)] * len(captured) and okg == 0, codes
    assert _bits(ok) == _bits(index.search_reweighted(q[:2], 5))

    # after the whole table: the index answers as before it
    assert _bits(index.search_reweighted(q[:40], 10)) + _bits(index.search_masked(q[:40], 10, mask)) == before
    for h in (other_grouping, other_fusion, view_fusion):
        h.close()


# ---- c. a grouping does not outlive its index's identity ---------------------------------------------------------------------
def test_the_grouping_of_a_closed_and_recreated_index_is_refused():
    s = _setup()
    first = IcdIndex(s["corpus"], s["levels"], max_nq=16, max_k=16)
    grouping = first.grouping(s["group_of"], max_nq=8)
    address = first._h.value
    first.close()
    again = IcdIndex(s["corpus"], s["levels"], max_nq=16, max_k=16)   # the same n, dim and device; often the same address
    try:
        if again._h.value == address:
            with pytest.raises(_native.IcdError) as e:
                again.search_grouped(s["q"][:2], 2, 2, grouping)
            assert e.value.code == -1 and "another index" in str(e.value)
        else:
            print("vacuous: the re-created index did not reuse the closed one's address, the owner comparison alone refuses")
            with pytest.raises(_native.IcdError):
                again.search_grouped(s["q"][:2], 2, 2, grouping)
    finally:
        grouping.close()
        again.close()
