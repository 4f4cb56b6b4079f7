"""icd_index_search_wide on the device against tests/wide_oracle.py over the CPU oracle's full ranking, byte
for byte: raw and reweighted outputs, count and selected; no tolerance anywhere. dim 32 unless stated. Sizes sit at the sweep's
128-row tile (1, 129, 257, 4 097), the collect's 1 024-row step and the sort's tiers (k = 1 024 | 1 025, 4 096 | 4 097, 16 384);
batches at the sweep's 128-query tile (127, 128, 129, 300)."""
import ctypes

import numpy as np
import pytest

import wide_oracle as wo
from conftest import icd_levels, unit_rows
from rag_project_icd10_amd import _native

pytestmark = pytest.mark.gpu

BASE = 5_000_000_000
KS = (1, 128, 129, 256, 257, 1000, 1024, 1025, 4096, 4097, 16384)
NQS = (1, 5, 127, 128, 129, 300)


def same(got, want, what):
    """arrays compared byte for byte"""
    assert len(got) == len(want), what
    for j, (g, w) in enumerate(zip(got, want)):
        g = np.asarray(g)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, j, g.dtype, w.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (what, j, g, w)


class Case:
    """one corpus on the device, a fixed query batch and the oracle's full ranking of it (computed once, never changed)"""

    def __init__(self, orc, corpus, queries, levels=None, id_base=0, ws_nq=None, ws_k=wo.MAX_K):
        self.corpus, self.queries, self.id_base = corpus, np.ascontiguousarray(queries, np.float32), id_base
        self.n, self.dim = corpus.shape
        self.levels = icd_levels(self.n, self.n + 1) if levels is None else np.asarray(levels, np.int32)
        self.index = _native.IcdIndex(corpus, self.levels, device=0, max_nq=512, max_k=128, id_base=id_base, probe=False)
        self.ws = _native.IcdWide(self.index, len(self.queries) if ws_nq is None else ws_nq, ws_k)
        self.fs, self.fi = orc.flat_ip_topk(corpus, self.queries, self.n, id_base=id_base)
        self.handles = {}

    def handle(self, mask):
        if mask is None:
            return None
        if id(mask) not in self.handles:
            self.handles[id(mask)] = (mask, self.index.rowmask(np.nonzero(mask)[0].astype(np.int64)))
        return self.handles[id(mask)][1]

    def check(self, k, nq=None, first=0, masks=None, radius=None, range_filter=None, forms=(False, True)):
        """both forms of one call against the oracle; returns the oracle's (raw, adj, count, selected)"""
        nq = len(self.queries) if nq is None else nq
        want = wo.wide_batch(self.fs[:nq], self.fi[:nq], self.levels, k, first, masks, radius, range_filter, self.id_base)
        hm = None if masks is None else [self.handle(m) for m in masks]
        what = (self.n, self.dim, nq, k, first)
        for rew in forms:
            got = self.ws.search_wide(self.queries[:nq], k, masks=hm, radius=radius, range_filter=range_filter, first=first, reweighted=rew)
            if rew:
                same(got[:4], want[1], what + ("reweighted",))
            else:
                assert got[0] is None
                same(got[1:4], want[0], what + ("raw",))
            same(got[4:], want[2:], what + ("count, selected", rew))
        return want

    def close(self):
        for _m, h in self.handles.values():
            h.close()
        self.ws.close()
        self.index.close()


def family_corpus(n, dim, seed):
    """families of 1 .. 5 bit-identical rows: their members tie, the smaller id first"""
    rng = np.random.default_rng(seed)
    fam = np.repeat(np.arange(n), rng.integers(1, 6, n))[:n]
    return np.ascontiguousarray(unit_rows(n, dim, seed)[fam])


# ---- the shape grid ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t,n", list(enumerate((1, 129, 257, 1000, 4097, 16500))))
def test_shape_grid(oracle, t, n):
    """every n with every k (k > n pads), the batch sizes in turn; an id_base on every other corpus"""
    case = Case(oracle, family_corpus(n, 32, 100 + n), unit_rows(300, 32, 7 * n), id_base=BASE if t % 2 else 0)
    try:
        for j, k in enumerate(KS):
            nq = NQS[(j + t) % len(NQS)]
            raw, _adj, count, selected = case.check(k, nq=nq)
            assert (count == min(k, n)).all() and (selected == n).all() and (raw[1][:, min(k, n):] == -1).all()
    finally:
        case.close()


def test_dim_768_and_more_than_one_score_block(oracle):
    case = Case(oracle, family_corpus(1500, 768, 5), unit_rows(130, 768, 6), id_base=BASE)
    try:
        case.check(1000)
        case.check(129, nq=3, first=500)
    finally:
        case.close()
    # a workspace of 7 queries: the ctypes layer cuts the batch into calls of 7. And one call whose score block holds fewer
    # queries than the call: 2 304 queries x (n padded x 4 + 16 384 x 32 bytes) exceeds the 256 MiB budget
    case = Case(oracle, family_corpus(300, 32, 8), unit_rows(20, 32, 9), ws_nq=7)
    try:
        case.check(257)
    finally:
        case.close()
    nq = 600
    case = Case(oracle, family_corpus(300, 32, 8), unit_rows(nq, 32, 10), ws_nq=nq)
    try:
        assert case.ws.stats()["bytes"] < (300 << 20)   # (the blocks of 384 queries, not nq x max_k outputs)
        case.check(300)
    finally:
        case.close()


# ---- k <= 128 equals the existing searches ---------------------------------------------------------------------------------------
def test_small_k_equals_the_existing_searches(oracle):
    n, nq = 1000, 40
    case = Case(oracle, family_corpus(n, 32, 21), unit_rows(nq, 32, 22), id_base=77)
    try:
        rng = np.random.default_rng(1)
        masks = [None if q % 4 == 0 else rng.random(n) < 0.5 for q in range(nq)]
        hm = [case.handle(m) for m in masks]
        lo, hi = case.fs[:, 300].copy(), case.fs[:, 20].copy()
        for k in (1, 10, 128):
            for rew in (False, True):
                cut = slice(0 if rew else 1, 4)
                for kw in ({}, {"radius": lo, "range_filter": hi}):
                    got = case.ws.search_wide(case.queries, k, reweighted=rew, **kw)
                    same(got[cut], case.index.search_range(case.queries, k, reweighted=rew, **kw), ("range", k, rew))
                    got = case.ws.search_wide(case.queries, k, masks=hm, reweighted=rew, **kw)
                    same(got[cut], case.index.search_masked(case.queries, k, hm, reweighted=rew, **kw), ("masked", k, rew))
    finally:
        case.close()


# ---- ties at the cut ---------------------------------------------------------------------------------------------------------------
def test_ties_at_the_cut(oracle):
    rows8 = unit_rows(8, 32, 31)
    case = Case(oracle, np.ascontiguousarray(np.tile(rows8, (250, 1))), unit_rows(5, 32, 32))   # every score has 250 copies
    try:
        for k in (129, 250, 251, 1000):
            raw = case.check(k)[0]
            for q in range(5):   # within one score the kept ids are the smallest, ascending
                for s in np.unique(raw[0][q]):
                    ids = raw[1][q][raw[0][q] == s]
                    assert (np.diff(ids) == 8).all() and ids[0] < 8
    finally:
        case.close()
    case = Case(oracle, np.ascontiguousarray(np.tile(rows8[:1], (2000, 1))), unit_rows(3, 32, 33), id_base=BASE)
    try:
        for k in (129, 1024):
            raw = case.check(k)[0]
            assert (raw[1] == BASE + np.arange(k)).all()
    finally:
        case.close()


# ---- every digit of the radix select -----------------------------------------------------------------------------------------------
def test_every_digit_of_the_radix_select(oracle):
    e0 = np.zeros(32, np.float32)
    e0[0] = 1.0
    low = np.zeros((4096, 32), np.float32)
    low[:, 0] = np.float32(1.0) + np.arange(4096, dtype=np.float32) * np.float32(2.0 ** -23)   # scores differ in the lowest 12 bits only
    perm = np.random.default_rng(41).permutation(4096)
    case = Case(oracle, np.ascontiguousarray(low[perm]), e0[None, :])
    try:
        assert len(np.unique(case.fs[0])) == 4096 and len(np.unique(wo.order_u32(case.fs[0]) >> 12)) == 1
        for k in (1, 129, 1000, 1025, 3000, 4095, 4096):
            case.check(k)
        case.check(200, first=2000)
    finally:
        case.close()
    # sign and exponent only: +- 2^e, every mantissa zero - the scores differ in the top digit (and one bit of the second)
    exps = np.arange(-60, 60)
    top = np.zeros((240, 32), np.float32)
    top[:120, 0], top[120:, 0] = np.ldexp(np.float32(1.0), exps), -np.ldexp(np.float32(1.0), exps)
    case = Case(oracle, np.ascontiguousarray(np.tile(top, (3, 1))), e0[None, :])
    try:
        assert len(np.unique(wo.order_u32(case.fs[0]) & np.uint32((1 << 23) - 1))) <= 2
        for k in (1, 100, 129, 361, 500, 720):
            case.check(k)
    finally:
        case.close()


# ---- special scores -----------------------------------------------------------------------------------------------------------------
def test_special_scores(oracle):
    n = 700
    x = family_corpus(n, 32, 51)
    tiny = np.finfo(np.float32).tiny
    x[10:40] = 0.0                                   # +0.0 scores ...
    x[40:70, 0] = np.float32(-1e-30)                 # ... and tiny products of either sign around them
    x[40:70, 1:] = 0.0
    x[70:100, 0], x[70:100, 1:] = tiny, 0.0          # subnormal scores for |q0| < 1
    x[100:110, 3] = np.nan                           # NaN rows: in no list
    x[110:115, 0], x[110:115, 1:] = np.inf, 0.0      # +-inf scores (the sign of q0 decides)
    x[115:120, 0], x[115:120, 1:] = -np.inf, 0.0
    x[120:130] = -0.0
    q = unit_rows(6, 32, 52)
    q[1] = np.abs(q[1])
    q[2, 0] = 0.0                                    # inf x 0: NaN scores on rows 110 .. 119 as well
    case = Case(oracle, x, q)
    try:
        for k in (129, 600, 700, 1025):
            _raw, _adj, _count, selected = case.check(k)
            assert (selected[[0, 1, 3, 4, 5]] == n - 10).all() and selected[2] == n - 20
        m = np.zeros(n, bool)
        m[90:125] = True
        assert (case.check(129, masks=[m] * 6)[3][[0, 1]] == 25).all()
    finally:
        case.close()


# ---- masks ----------------------------------------------------------------------------------------------------------------------------
def test_masks(oracle):
    n, k, nq = 1100, 200, 8
    case = Case(oracle, family_corpus(n, 32, 61), unit_rows(nq, 32, 62), id_base=BASE)
    try:
        rng = np.random.default_rng(63)

        def admitting(m):
            out = np.zeros(n, bool)
            out[rng.choice(n, m, replace=False)] = True
            return out
        tail = np.zeros(n, bool)
        tail[1024 + 5:] = True                       # all in the last, partial tile (rows 1 024 .. 1 099)
        masks = [admitting(0), admitting(1), admitting(k - 1), admitting(k), admitting(k + 1), tail, None, admitting(n)]
        _raw, _adj, count, selected = case.check(k, masks=masks)
        assert selected.tolist() == [0, 1, k - 1, k, k + 1, n - 1029, n, n] and count.tolist() == [0, 1, k - 1, k, k, n - 1029, k, k]
        case.check(1025, masks=masks)
        case.check(50, first=180, masks=masks)
    finally:
        case.close()


# ---- bands ----------------------------------------------------------------------------------------------------------------------------
def test_bands(oracle):
    n, nq = 1500, 6
    case = Case(oracle, family_corpus(n, 32, 71), unit_rows(nq, 32, 72))
    try:
        # bounds equal to scores that occur: radius is strict, range_filter inclusive
        lo, hi = case.fs[:, 900].copy(), case.fs[:, 30].copy()
        raw = case.check(1000, radius=lo, range_filter=hi)[0]
        for q in range(nq):
            real = raw[0][q][raw[1][q] >= 0]
            assert real[0].tobytes() == hi[q].tobytes() and real[-1] > lo[q] and (case.fs[q] == lo[q]).any()
        case.check(129, radius=float(np.median(case.fs)))                      # one scalar for every query
        _raw, _adj, count, selected = case.check(500, radius=case.fs[:, 140].copy())   # fewer than k rows in the band
        assert (count == selected).all() and (count < 500).all() and (count > 0).all()
        m = np.random.default_rng(73).random(n) < 0.5
        case.check(400, first=100, masks=[m, None] * 3, radius=lo, range_filter=hi)
    finally:
        case.close()


# ---- first ------------------------------------------------------------------------------------------------------------------------------
def test_first(oracle):
    n, nq = 16500, 3
    case = Case(oracle, family_corpus(n, 32, 81), unit_rows(nq, 32, 82), id_base=3)
    try:
        case.check(384, first=16000)                 # first + k = 16 384
        case.check(1, first=16383)
        whole = case.ws.search_wide(case.queries, 1300, reweighted=False)
        part = case.ws.search_wide(case.queries, 300, first=1000, reweighted=False)
        same([p[:, :] for p in part[1:4]], [np.ascontiguousarray(w[:, 1000:]) for w in whole[1:4]], "the slice of first = 0")
        m = np.zeros(n, bool)
        m[:50] = True
        _raw, _adj, count, selected = case.check(129, first=50, masks=[m] * nq)     # first past the last ranking row
        assert (count == 0).all() and (selected == 50).all()
        case.check(129, first=49, masks=[m] * nq)
    finally:
        case.close()


# ---- reweighting ------------------------------------------------------------------------------------------------------------------------
def test_reweighting_levels_and_equal_adj_across_classes(oracle):
    n = 3000
    rng = np.random.default_rng(91)
    levels = rng.choice(np.array([0, 1, 2, 3, 7], np.int32), n)
    case = Case(oracle, family_corpus(n, 32, 92), unit_rows(4, 32, 93), levels=levels)
    try:
        for k in (129, 1025, 3000):
            case.check(k, forms=(True,))
    finally:
        case.close()
    # pairs whose doubles collide: a at level 2 (weight 1.0) and b at level 1 with float64(b) * 1.2 == float64(a), found on the CPU
    # (b = 5 m / 1024, a = 6 m / 1024: the double nearest 1.2 is off by less than half an ulp of the product)
    pairs = [(np.float32(6 * m / 1024), np.float32(5 * m / 1024)) for m in range(1, 101)]
    assert all(np.float64(a) == np.float64(b) * 1.2 for a, b in pairs)
    x = np.zeros((400, 32), np.float32)
    lv = np.zeros(400, np.int32)
    for j, (a, b) in enumerate(pairs):               # b (level 1) at the smaller and at the larger row of a's (level 2)
        x[4 * j, 0], x[4 * j + 1, 0], x[4 * j + 2, 0], x[4 * j + 3, 0] = b, a, a, b
        lv[4 * j:4 * j + 4] = (1, 2, 2, 1)
    e0 = np.zeros((1, 32), np.float32)
    e0[0, 0] = 1.0
    case = Case(oracle, x, e0, levels=lv)
    try:
        adj = case.check(400, forms=(True,))[1]
        assert len(np.unique(adj[0][0])) == 100      # the doubles do collide: four hits to every adj
        for k in (129, 200):
            case.check(k, forms=(True,))
    finally:
        case.close()


# ---- determinism, device tensors ------------------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bytes_and_device_tensors(oracle):
    import torch
    n, nq = 5000, 129
    case = Case(oracle, family_corpus(n, 32, 95), unit_rows(nq, 32, 96))
    try:
        m = np.random.default_rng(97).random(n) < 0.7
        hm = [case.handle(m)] * nq
        first_run = case.ws.search_wide(case.queries, 4097, masks=hm, radius=-0.2)
        for _ in range(2):
            same(case.ws.search_wide(case.queries, 4097, masks=hm, radius=-0.2), first_run, "second run")
        dq = torch.from_numpy(case.queries).cuda()
        dev = case.ws.search_wide(dq, 4097, masks=hm, radius=torch.full((nq,), -0.2, device="cuda"))
        assert all(t.is_cuda for t in dev)
        same([t.cpu().numpy() for t in dev], first_run, "device tensors")
        raw = case.ws.search_wide(dq, 300, reweighted=False)
        want = wo.wide_batch(case.fs, case.fi, case.levels, 300)
        assert raw[0] is None
        same([t.cpu().numpy() for t in raw[1:4]], want[0], "device raw")
    finally:
        case.close()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals(oracle):
    lib = _native.load_library()
    case = Case(oracle, family_corpus(300, 32, 98), unit_rows(4, 32, 99), ws_nq=4, ws_k=1000)
    other = _native.IcdIndex(case.corpus, case.levels, device=0, max_nq=64, max_k=128, probe=False)
    view = case.index.view(np.arange(0, 300, 2, dtype=np.int64))
    try:
        k_out = 1000
        outs = [np.full((4, k_out), 7, dt) for dt in (np.float64, np.float32, np.int64, np.int32)] + [np.full(4, 7, np.int32), np.full(4, 7, np.int64)]
        p = [o.ctypes.data for o in outs]

        def call(index=case.index, ws=case.ws, nq=4, k=10, first=0, rew=1, out=p):
            return lib.icd_index_search_wide(index._h, ws._h, None, case.queries.ctypes.data, nq, k, first, 0, None, None, 0, rew, *out, 0, None)

        assert call() == 0
        untouched = [o.copy() for o in outs]
        for kw in (dict(k=0), dict(k=16385), dict(first=-1), dict(first=16000, k=385), dict(k=1001), dict(first=1, k=1000), dict(nq=5), dict(nq=-1),
                   dict(index=other), dict(out=[None] + p[1:]), dict(out=p[:1] + [None] + p[2:]), dict(out=p[:4] + [None, p[5]]), dict(out=p[:5] + [None])):
            assert call(**kw) == -1, kw
        assert call(index=view) == -4                                       # a view: ICD_ERR_UNSUPPORTED
        for o, u in zip(outs, untouched):                                   # a refused call writes no output
            assert o.tobytes() == u.tobytes()
        assert call(rew=0, out=[None] + p[1:]) == 0                       # out_adj may be NULL in the raw form
        h = ctypes.c_void_p()
        assert lib.icd_wide_create(view._h, 4, 100, ctypes.byref(h)) == -4 and not h.value
        assert lib.icd_wide_create(case.index._h, 0, 100, ctypes.byref(h)) == -1 and lib.icd_wide_create(case.index._h, 4, 16385, ctypes.byref(h)) == -1
        gone = _native.IcdWide(case.index, 4, 100)
        stale = ctypes.c_void_p(gone._h.value)
        gone.close()
        assert lib.icd_index_search_wide(case.index._h, stale, None, case.queries.ctypes.data, 4, 10, 0, 0, None, None, 0, 1, *p, 0, None) == -5
        assert lib.icd_wide_destroy(stale) == -5
        # the ctypes layer's own checks
        for bad in (dict(k=0), dict(k=16385), dict(k=10, first=-1), dict(k=385, first=16000)):
            with pytest.raises(ValueError):
                case.ws.search_wide(case.queries, **bad)
        with pytest.raises(_native.IcdError):
            case.ws.search_wide(case.queries, 10, radius=0.5, range_filter=0.25)     # an inverted host band
        assert case.ws.stats()["max_nq"] == 4 and case.ws.stats()["max_k"] == 1000
    finally:
        view.close()
        other.close()
        case.close()
