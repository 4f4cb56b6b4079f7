"""Range, masked, grouped and hybrid search OFF the one shape the other modules test them at (run with -m gpu on an MI355X):
every list width of the band and mask kernels (KP 16 / 32 / 64 / 128) at every batch tier, other dims than 768, corpora of a
tile or less, id_base != 0 and degenerate score distributions. Everything is compared with the numpy walkers (range_oracle,
mask_oracle, grouped_oracle, hybrid_oracle) over the oracle's FULL ranking - oracle.flat_ip_topk(corpus, q, n, id_base=...) -
byte for byte over every output array, raw and reweighted; no tolerance anywhere. Every case asserts its own precondition on the
oracle's side before the device is touched. DESIGN.md sections 11 and 12 map the kernel instantiations to the cases here."""
import numpy as np
import pytest

from conftest import icd_levels, unit_rows
from grouped_oracle import Ranking, expected
from hybrid_oracle import fuse_query, hybrid_batch
from mask_oracle import masked_batch
from range_oracle import band_batch, in_band, pages
from test_grouped_search_gpu import N, NQ
from test_range_search_gpu import _parent

pytestmark = pytest.mark.gpu

from rag_project_icd10_amd._native import MODE_EXACT, IcdIndex  # noqa: E402

ROWS = np.arange(N, dtype=np.int64)
HALF = ((ROWS * 2654435761) >> 7) & 1 == 1


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else a


def _bits(a):
    return np.ascontiguousarray(_np(a)).tobytes()


def _same(got, want, nq, what):
    """every output array of a call against the first nq rows of the oracle's: dtype, shape and bytes"""
    assert len(got) == len(want), what
    for j, (g, w) in enumerate(zip(got, want)):
        g, w = _np(g), w[:nq]
        if g.dtype == np.int32 and w.dtype == np.uint32:   # (request bits come back as an int32 tensor from the device)
            g = g.view(np.uint32)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, j, g.dtype, w.dtype, g.shape, w.shape)
        assert _bits(g) == _bits(w), (what, "array", j, "nq", nq, "queries", np.nonzero((g != w).any(1))[0][:5])


def _cut(v, nq, dev):
    if v is None:
        return None
    if isinstance(v, tuple):
        return tuple(_cut(x, nq, dev) for x in v)
    v = v[:nq] if hasattr(v, "__len__") else v
    if dev and hasattr(v, "__len__"):
        import torch
        return torch.from_numpy(np.ascontiguousarray(v)).cuda()
    return v


def _banded(index, q, want, k, nq, what, masks=None, dev=False, **bounds):
    """search_range (masks None) or search_masked of the first nq queries, raw and reweighted, against band_batch's /
    masked_batch's result; dev: queries and bounds as device tensors (the band_pack_kernel path)"""
    b = {name: _cut(v, nq, dev) for name, v in bounds.items()}
    qs = _cut(q, nq, dev)
    out = []
    for rew, exp in ((False, want[0]), (True, want[1])):
        got = index.search_range(qs, k, reweighted=rew, **b) if masks is None else index.search_masked(qs, k, masks[:nq], reweighted=rew, **b)
        _same(got, exp, nq, (what, "reweighted" if rew else "raw", k))
        out += [_bits(g) for g in got]
    return out


class _Masks:
    """device masks of boolean selections, made once per selection and closed with the test"""

    def __init__(self, index):
        self.index, self.made = index, {}

    def __call__(self, sel):
        if sel is None:
            return None
        key = sel.tobytes()
        if key not in self.made:
            self.made[key] = self.index.rowmask(np.nonzero(sel)[0])
        return self.made[key]

    def close(self):
        for m in self.made.values():
            m.close()
        self.made = {}


# ---- 1. every list width, every tier --------------------------------------------------------------------------------------------
WIDTH_KS = (16, 17, 32, 33, 64, 65)                        # KP 16 | 32 | 32 | 64 | 64 | 128
# single launch at k <= 16 (1 .. 4) | QB = 8 streaming (5, 8) | a pass of eight and a pass of one (9) | 40 | ST_MAX_ACTIVE (64) | the
# first MFMA batch (65) | a second query tile of the four-wave MFMA form with 127 dead slots (129) | 300
TIERS = (1, 2, 3, 4, 5, 8, 9, 40, 64, 65, 129, 300)
NEUTRAL = (np.float32(np.inf), 0)                          # a cursor every finite score lies behind


def _width_cases(s_all, i_all, k):
    """{name: bounds}: ceiling at rank 200, floor at rank max(k - 3, 5), both, a cursor on a member of a duplicate pair (even
    queries: the lower id, odd queries: the higher), and a per-query mix of the four"""
    nq = len(s_all)
    qs = np.arange(nq)
    ceiling, floor = s_all[:, 200].copy(), s_all[:, max(k - 3, 5)].copy()
    lo2 = s_all[:, 260].copy()
    cur = (s_all[qs, qs % 2].copy(), i_all[qs, qs % 2].copy())
    kind = qs % 4
    mix_lo = np.where(kind == 1, floor, np.where(kind == 2, lo2, -np.inf)).astype(np.float32)
    mix_hi = np.where((kind == 0) | (kind == 2), ceiling, np.inf).astype(np.float32)
    mix_cur = (np.where(kind == 3, cur[0], NEUTRAL[0]).astype(np.float32), np.where(kind == 3, cur[1], NEUTRAL[1]).astype(np.int64))
    return {"ceiling": {"range_filter": ceiling}, "floor": {"radius": floor}, "both": {"radius": lo2, "range_filter": ceiling},
            "cursor": {"after": cur}, "mix": {"radius": mix_lo, "range_filter": mix_hi, "after": mix_cur}}


def _width_preconditions(name, want, s_all, i_all, k):
    ids = want[0][1]
    n_hits = (ids >= 0).sum(1)
    pair = np.arange(40)   # queries 0 .. 39 ARE rows 5000 + 2 j, whose twin is row 5001 + 2 j
    if name == "ceiling":   # a post-filter of the ordinary search cannot answer: no hit lies in the plain top-128, every list is full
        assert (n_hits == k).all()
        assert not any(set(ids[r].tolist()) & set(i_all[r, :128].tolist()) for r in range(len(ids)))
    elif name == "floor":   # lists come out short
        assert (n_hits <= max(k - 3, 5)).all() and (n_hits < k).all() and (n_hits == max(k - 3, 5)).mean() > 0.8
    elif name == "both":
        # ranks 200 .. 259, one more or less where a duplicate pair straddles an end: short lists at k >= 64
        assert (s_all[:, 260] < s_all[:, 200]).all() and (n_hits <= 61).all() and (n_hits == min(k, 60)).mean() > 0.8
    elif name == "cursor":
        assert (i_all[pair, 0] == 5000 + 2 * pair).all() and (i_all[pair, 1] == 5001 + 2 * pair).all()
        assert _bits(s_all[pair, 0]) == _bits(s_all[pair, 1])
        assert (ids[pair[0::2], 0] == 5001 + 2 * pair[0::2]).all()                  # behind the lower id: the twin comes first
        assert not (ids[pair[1::2]] == 5001 + 2 * pair[1::2, None]).any()           # behind the higher id: the twin is gone
        assert (ids[pair[1::2], 0] == i_all[pair[1::2], 2]).all() and (n_hits == k).all()


@pytest.mark.parametrize("k", WIDTH_KS)
@pytest.mark.parametrize("kind", ["gauss", "family"])
def test_range_search_at_every_list_width_and_tier(oracle, kind, k):
    corpus, levels, q, index, s_all, i_all = _parent(kind, oracle)
    for name, bounds in _width_cases(s_all, i_all, k).items():
        want = band_batch(s_all, i_all, levels, k, **bounds)
        _width_preconditions(name, want, s_all, i_all, k)
        for nq in TIERS:
            _banded(index, q, want, k, nq, (kind, name), **bounds)
    # rule 6: no bound at all = the MODE_EXACT search, bit for bit
    for nq in TIERS:
        ps, pi = index.search(q[:nq], k, MODE_EXACT)
        g_raw = index.search_range(q[:nq], k, reweighted=False)
        assert _bits(g_raw[0]) == _bits(ps) and _bits(g_raw[1]) == _bits(pi), nq
        assert [_bits(t) for t in index.search_range(q[:nq], k)] == [_bits(t) for t in index.search_reweighted(q[:nq], k, MODE_EXACT)], nq


def _width_masks(name, bounds, s_all, i_all, k, which):
    """per-query selections: one shared mask of 5 % of the rows | per query exactly k - 1 rows of its band (fewer only where the
    band itself is smaller) next to 64 rows outside it | per-query masks with None entries"""
    nq = len(s_all)
    if which == "shared":
        return [ROWS % 20 == 7] * nq
    if which == "mixed":
        return [None if r % 3 == 0 else (ROWS % 20 == r % 20 if r % 3 == 1 else HALF) for r in range(nq)]
    rng = np.random.default_rng(1000 * k + len(name))
    sels = []
    for r in range(nq):
        b = {n_: (v[r] if not isinstance(v, tuple) else (v[0][r], v[1][r])) for n_, v in bounds.items()}
        band = in_band(s_all[r], i_all[r], **b)
        inside, outside = i_all[r][band], i_all[r][~band]
        sel = np.zeros(N, bool)
        sel[rng.choice(inside, min(k - 1, len(inside)), replace=False)] = True
        sel[rng.choice(outside, min(64, len(outside)), replace=False)] = True
        sels.append(sel)
    return sels


@pytest.mark.parametrize("k", WIDTH_KS)
@pytest.mark.parametrize("kind", ["gauss", "family"])
def test_masked_search_at_every_list_width_and_tier(oracle, kind, k):
    corpus, levels, q, index, s_all, i_all = _parent(kind, oracle)
    mk = _Masks(index)
    try:
        for name, bounds in _width_cases(s_all, i_all, k).items():
            for which in ("shared", "k-1", "mixed"):
                sels = _width_masks(name, bounds, s_all, i_all, k, which)
                want = masked_batch(s_all, i_all, levels, sels, k, **bounds)
                n_hits = (want[0][1] >= 0).sum(1)
                if which == "shared" and name in ("ceiling", "cursor"):
                    assert int(sels[0].sum()) == N // 20 and (n_hits == k).all()     # every query has at least k masked rows in the band
                if which == "k-1":
                    full = np.array([int(in_band(s_all[r], i_all[r], **{n_: (v[r] if not isinstance(v, tuple) else (v[0][r], v[1][r]))
                                                                         for n_, v in bounds.items()}).sum()) for r in range(NQ)])
                    assert (n_hits == np.minimum(k - 1, full)).all() and (want[0][1][:, -1] == -1).all()
                    if name in ("ceiling", "cursor"):
                        assert (n_hits == k - 1).all()
                dev = [mk(s) for s in sels]
                for nq in TIERS:
                    _banded(index, q, want, k, nq, (kind, name, which), masks=dev, **bounds)
                mk.close()
        # rule 6 of section 12: a mask of every row = no mask = the MODE_EXACT search
        full = [mk(np.ones(N, bool))] * NQ
        for nq in TIERS:
            plain = index.search_range(q[:nq], k, reweighted=False)
            got = index.search_masked(q[:nq], k, full[:nq], reweighted=False)
            assert [_bits(t) for t in got] == [_bits(t) for t in plain], nq
            ps, pi = index.search(q[:nq], k, MODE_EXACT)
            assert _bits(got[0]) == _bits(ps) and _bits(got[1]) == _bits(pi), nq
            assert [_bits(t) for t in index.search_masked(q[:nq], k, full[:nq])] == [_bits(t) for t in index.search_reweighted(q[:nq], k, MODE_EXACT)], nq
    finally:
        mk.close()


@pytest.mark.parametrize("kind", ["gauss", "family"])
def test_general_streaming_form_at_k16_without_the_single_launch(oracle, kind):
    """up to 4 queries at k <= 16 take the single-launch kernel; with the stream_one option off the same calls run
    launch_stream<16, 2, 1 | 2 | 4, BAND[, MASK]>: the same bytes as the first run, and as the oracle"""
    corpus, levels, q, index, s_all, i_all = _parent(kind, oracle)
    k = 16
    mk = _Masks(index)
    runs = []
    try:
        for option in (1, 0):
            index.set_option("stream_one", option)
            seen = []
            for name, bounds in _width_cases(s_all, i_all, k).items():
                want = band_batch(s_all[:4], i_all[:4], levels, k, **{n_: _cut(v, 4, False) for n_, v in bounds.items()})
                sels = [ROWS % 20 == 7, None, HALF, ROWS % 20 == 3]
                want_m = masked_batch(s_all[:4], i_all[:4], levels, sels, k, **{n_: _cut(v, 4, False) for n_, v in bounds.items()})
                dev = [mk(s) for s in sels]
                for nq in (1, 2, 3, 4):
                    for on_dev in (False, True):   # (a host caller's ONE query is the in-argument form when the option is on)
                        seen += _banded(index, q, want, k, nq, (kind, name, option), dev=on_dev, **bounds)
                        seen += _banded(index, q, want_m, k, nq, (kind, name, "masked", option), masks=dev, dev=on_dev, **bounds)
            for nq in (1, 2, 3, 4):
                seen += [_bits(t) for t in index.search_range(q[:nq], k, reweighted=False)[:2]]
                assert seen[-2:] == [_bits(t) for t in index.search(q[:nq], k, MODE_EXACT)]
            runs.append(seen)
    finally:
        index.set_option("stream_one", 1)
        mk.close()
    assert runs[0] == runs[1]


# ---- 2. other dims --------------------------------------------------------------------------------------------------------------
DIM_NQ = 70


def _dim_setup(dim, oracle, id_base=0):
    n = 700 if dim == 4096 else 2500
    x = unit_rows(n, dim, 40 + dim)
    x[501:560:2] = x[500:560:2]                                     # a block of duplicated rows
    rng = np.random.default_rng(dim)
    q = x[rng.integers(0, n, DIM_NQ - 10)] + (0.3 / np.sqrt(dim)) * rng.standard_normal((DIM_NQ - 10, dim)).astype(np.float32)
    q = np.ascontiguousarray(np.concatenate([x[500:520:2], q]), dtype=np.float32)   # queries 0 .. 9 ARE duplicated rows
    levels = icd_levels(n, dim)
    s_all, i_all = oracle.flat_ip_topk(x, q, n, id_base=id_base)
    return x, levels, q, s_all, i_all


@pytest.mark.parametrize("dim", [32, 96, 256, 1024, 2048, 4096])
def test_band_and_mask_at_other_dims(oracle, dim):
    """stream_fits lowers the queries per pass as dim grows, plan_stream_one refuses large dims, a host caller's ONE query travels
    in the kernel arguments up to 768 floats and is copied above, nks = dim / 32 runs from 1 to 128"""
    corpus, levels, q, s_all, i_all = _dim_setup(dim, oracle)
    n = len(corpus)
    rows = np.arange(n)
    pair = np.arange(10)
    assert (i_all[pair, 0] == 500 + 2 * pair).all() and (i_all[pair, 1] == 501 + 2 * pair).all() and _bits(s_all[pair, 0]) == _bits(s_all[pair, 1])
    index = IcdIndex(corpus, levels, max_nq=128, max_k=128)
    sel = rows % 3 == 1
    mask = index.rowmask(np.nonzero(sel)[0])
    try:
        ceiling = {"range_filter": s_all[:, 200].copy()}
        floor_cur = {"radius": s_all[:, 30].copy(), "after": (s_all[:, 0].copy(), i_all[:, 0].copy())}   # a cursor ON the lower twin
        for k in (10, 20, 50, 128):
            w_ceil = band_batch(s_all, i_all, levels, k, **ceiling)
            assert (w_ceil[0][1] >= 0).all() and not any(set(w_ceil[0][1][r].tolist()) & set(i_all[r, :128].tolist()) for r in range(DIM_NQ))
            w_fc = band_batch(s_all, i_all, levels, k, **floor_cur)
            assert (w_fc[0][1][pair, 0] == 501 + 2 * pair).all() and ((w_fc[0][1] >= 0).sum(1) <= 29).all()
            w_mask = masked_batch(s_all, i_all, levels, [sel] * DIM_NQ, k, **ceiling)
            assert ((w_mask[0][1] >= 0).sum(1) == k).all() and sel[w_mask[0][1]].all()
            for nq in (1, 2, 4, 8, 40, 64, 65, 70):
                for on_dev in (False, True):
                    _banded(index, q, w_ceil, k, nq, (dim, "ceiling", on_dev), dev=on_dev, **ceiling)
                    _banded(index, q, w_fc, k, nq, (dim, "floor + cursor", on_dev), dev=on_dev, **floor_cur)
                    _banded(index, q, w_mask, k, nq, (dim, "mask", on_dev), masks=[mask] * DIM_NQ, dev=on_dev, **ceiling)
    finally:
        mask.close()
        index.close()


# ---- 3. corpus edges ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 7, 127, 128, 129, 257])
def test_corpora_of_a_tile_or_less(oracle, n):
    """a single partial tile (the first-tile bootstrap must not run), exactly one tile, one row more, two tiles and a row; k > n;
    a bitset of exactly four words (n <= 128); padding is exactly (-inf, -1, 0)"""
    dim, nq_all = 768, 65
    corpus, levels = unit_rows(n, dim, 700 + n), icd_levels(n, 701 + n)
    q = unit_rows(nq_all, dim, 702 + n)
    s_all, i_all = oracle.flat_ip_topk(corpus, q, n)
    assert (i_all >= 0).all()
    by_row = np.empty_like(s_all)
    np.put_along_axis(by_row, i_all, s_all, 1)               # by_row[q, r]: query q's score of row r
    last, first = by_row[:, n - 1].copy(), by_row[:, 0].copy()
    index = IcdIndex(corpus, levels, max_nq=128, max_k=128)
    mk = _Masks(index)
    only = lambda r: np.arange(n) == r
    cases = [("all", {"radius": np.float32(-3.0), "range_filter": np.float32(3.0)}, None),
             ("none", {"radius": s_all[:, 0].copy()}, None),
             ("only the last row", {"radius": np.nextafter(last, np.float32(-np.inf)), "range_filter": last}, None),
             ("cursor on the last row", {"after": (last, np.full(nq_all, n - 1, np.int64))}, None),
             ("cursor on the first row", {"after": (first, np.zeros(nq_all, np.int64))}, None),
             ("mask: the last row", {}, only(n - 1)), ("mask: row 0", {}, only(0)), ("mask: empty", {}, np.zeros(n, bool)),
             ("mask: every row", {}, np.ones(n, bool))]
    try:
        for name, bounds, sel in cases:
            for k in (1, 10, 32, 128):
                if sel is None:
                    want = band_batch(s_all, i_all, levels, k, **bounds)
                else:
                    want = masked_batch(s_all, i_all, levels, [sel] * nq_all, k, **bounds)
                raw, ids, lv = want[0]
                n_hits = (ids >= 0).sum(1)
                if name in ("all", "mask: every row"):
                    assert (n_hits == min(k, n)).all() and _bits(ids[:, :min(k, n)]) == _bits(i_all[:, :min(k, n)])
                elif name in ("none", "mask: empty"):
                    assert (n_hits == 0).all()
                elif name in ("only the last row", "mask: the last row"):
                    assert (n_hits == 1).all() and (ids[:, 0] == n - 1).all() and _bits(raw[:, 0]) == _bits(last)
                elif name == "mask: row 0":
                    assert (n_hits == 1).all() and (ids[:, 0] == 0).all()
                else:   # behind a row: the rows ranked behind it, of which there are n - 1 - its rank
                    rank = np.argmax(i_all == (n - 1 if "last" in name else 0), axis=1)
                    assert (n_hits == np.minimum(k, n - 1 - rank)).all()
                for nq in (1, 4, 9, 65):
                    for rew in (False, True):
                        masks = None if sel is None else [mk(sel)] * nq
                        got = (index.search_range(q[:nq], k, reweighted=rew, **{b: _cut(v, nq, False) for b, v in bounds.items()}) if sel is None
                               else index.search_masked(q[:nq], k, masks, reweighted=rew))
                        _same(got, want[1] if rew else want[0], nq, (n, name, k, rew))
                        g_ids = got[2] if rew else got[1]
                        pad = g_ids < 0
                        assert (g_ids[pad] == -1).all() and (got[-1][pad] == 0).all() and np.isneginf(got[0][pad]).all() and np.isneginf(got[1 if rew else 0][pad]).all()
                        assert (pad.sum(1) == k - n_hits[:nq]).all() and not pad[:, :1][n_hits[:nq] > 0].any()
    finally:
        mk.close()
        index.close()


# ---- 4. id_base -----------------------------------------------------------------------------------------------------------------
BASES = [1000, 2**32 + 12345]
N4, NQ4 = 3000, 80
ROWS4 = np.arange(N4, dtype=np.int64)
_CACHE4 = {}


def _corpus4():
    """3 000 unit rows with duplicate pairs at rows 2000 + 2j / 2001 + 2j; queries 0 .. 19 ARE rows 2000 + 2j, queries 20 + 3b + c are
    three noisy copies of base row b (requests built from them overlap partially)"""
    if "corpus" not in _CACHE4:
        x = unit_rows(N4, 768, 31)
        x[2001:2100:2] = x[2000:2100:2]
        rng = np.random.default_rng(32)
        base = x[rng.integers(0, N4, 20)]
        noisy = np.repeat(base, 3, axis=0) + 0.03 * rng.standard_normal((60, 768)).astype(np.float32)
        q = np.ascontiguousarray(np.concatenate([x[2000:2040:2], noisy]), dtype=np.float32)
        _CACHE4["corpus"] = (np.ascontiguousarray(x), icd_levels(N4, 33), q)
    return _CACHE4["corpus"]


def _based(id_base, oracle):
    if id_base not in _CACHE4:
        corpus, levels, q = _corpus4()
        s, i = oracle.flat_ip_topk(corpus, q, N4, id_base=id_base)
        assert i.min() == id_base and i.max() == id_base + N4 - 1
        _CACHE4[id_base] = (corpus, levels, q, IcdIndex(corpus, levels, max_nq=256, max_k=128, id_base=id_base), s, i)
    return _CACHE4[id_base]


def _untied_rank(s_all, start):
    """per query the first rank >= start whose score differs from both neighbours'"""
    return np.array([next(j for j in range(start, s_all.shape[1] - 1) if r[j - 1] > r[j] > r[j + 1]) for r in s_all])


@pytest.mark.parametrize("id_base", BASES)
def test_range_and_masked_search_with_an_id_base(oracle, id_base):
    corpus, levels, q, index, s_all, i_all = _based(id_base, oracle)
    pair, qs = np.arange(20), np.arange(NQ4)
    assert (i_all[pair, 0] == id_base + 2000 + 2 * pair).all() and (i_all[pair, 1] == id_base + 2001 + 2 * pair).all()
    c50, c110 = _untied_rank(s_all, 50), _untied_rank(s_all, 110)   # (a duplicate pair ties wherever it stands in a ranking)
    at50 = s_all[qs, c50].copy()
    below = np.where(qs % 2 == 0, id_base - 1 - qs, np.where(qs % 4 == 1, 5, -7)).astype(np.int64)   # (5 is BELOW both bases)
    cases = {"lower twin": {"after": (s_all[:, 0].copy(), i_all[:, 0].copy())},
             "higher twin": {"after": (s_all[:, 1].copy(), i_all[:, 1].copy())},
             "id below id_base": {"after": (at50, below)},
             "id at or above id_base + n": {"after": (at50, (id_base + N4 + (qs % 3) * 1000).astype(np.int64))},
             "cursor + band": {"after": (s_all[:, 70].copy(), i_all[:, 70].copy()), "radius": s_all[qs, c110].copy(), "range_filter": s_all[:, 60].copy()}}
    sel = ROWS4 % 7 == 3
    sels = [None if r % 3 == 0 else (sel if r % 3 == 1 else ROWS4 % 2 == 0) for r in range(NQ4)]
    mk = _Masks(index)
    try:
        dev_masks = [mk(s) for s in sels]
        for name, bounds in cases.items():
            for k in (10, 33, 128):
                want = band_batch(s_all, i_all, levels, k, id_base=id_base, **bounds)
                ids = want[0][1]
                if name == "lower twin":
                    assert (ids[pair, 0] == i_all[pair, 1]).all()
                elif name == "higher twin":
                    assert (ids[pair, 0] == i_all[pair, 2]).all() and not (ids[pair] == i_all[pair, 1][:, None]).any()
                elif name == "id below id_base":      # every row of the cursor's score passes: the page starts AT that rank
                    assert (ids[:, 0] == i_all[qs, c50]).all()
                elif name == "id at or above id_base + n":   # none does: it starts behind it
                    assert (ids[:, 0] == i_all[qs, c50 + 1]).all()
                else:                                 # ranks 71 .. c110 - 1
                    assert ((ids >= 0).sum(1) == np.minimum(k, c110 - 71)).all() and (ids[:, 0] == i_all[:, 71]).all()
                want_m = masked_batch(s_all, i_all, levels, sels, k, id_base=id_base, **bounds)
                assert all(sels[r] is None or sels[r][want_m[0][1][r][want_m[0][1][r] >= 0] - id_base].all() for r in range(NQ4))
                for nq in (1, 4, 9, 65, NQ4):
                    for on_dev in (False, True):
                        _banded(index, q, want, k, nq, (id_base, name, on_dev), dev=on_dev, **bounds)
                        _banded(index, q, want_m, k, nq, (id_base, name, "masked", on_dev), masks=dev_masks, dev=on_dev, **bounds)
    finally:
        mk.close()


@pytest.mark.parametrize("id_base", BASES)
def test_a_view_of_an_index_with_an_id_base(oracle, id_base):
    corpus, levels, q, index, _s, _i = _based(id_base, oracle)
    rows = np.arange(0, N4, 3, dtype=np.int64)
    view = index.view(rows)
    try:
        vs, vi = oracle.flat_ip_topk(corpus[rows], q, len(rows))
        gi = id_base + rows[vi]                                  # the view's hits carry the parent's ids
        assert (vs[:, 50] > vs[:, 51]).all() and (vs[:, 49] > vs[:, 50]).all()
        outside = gi[:, 50] + 1                                  # (row + 1 of a multiple of three: no row of the view)
        assert not np.isin(outside - id_base, rows).any()
        qs = np.arange(NQ4)
        cases = {"outside the view": ({"after": (vs[:, 50].copy(), outside)}, 51),
                 "just below a row of the view": ({"after": (vs[:, 50].copy(), gi[:, 50] - 1)}, 50),
                 "below id_base": ({"after": (vs[:, 50].copy(), np.where(qs % 2 == 0, id_base - 1, 7).astype(np.int64))}, 50),
                 "above every id": ({"after": (vs[:, 50].copy(), np.full(NQ4, id_base + N4 + 5, np.int64))}, 51),
                 "inside + ceiling": ({"after": (vs[:, 50].copy(), gi[:, 50].copy()), "range_filter": vs[:, 20].copy()}, 51)}
        for name, (bounds, first) in cases.items():
            for k in (10, 33, 128):
                want = band_batch(vs, gi, levels, k, id_base=id_base, **bounds)
                assert (want[0][1][:, 0] == gi[:, first]).all() and (want[0][1] >= 0).all()
                for nq in (1, 4, 9, 65, NQ4):
                    for on_dev in (False, True):
                        _banded(view, q, want, k, nq, (id_base, "view", name, on_dev), dev=on_dev, **bounds)
        group_of = (rows // 50).astype(np.int64)
        grouping = view.grouping(group_of)
        try:
            rk = Ranking(vs, vi, group_of)
            for k, s in ((10, 1), (10, 3), (1, 128)):
                want_raw, want_adj = expected(oracle, rk, levels, k, s, row_map=rows, id_base=id_base)
                for nq in (NQ4, 1, 17):
                    _same(view.search_grouped(q[:nq], k, s, grouping, reweighted=False), want_raw, nq, (id_base, "view grouped raw", k, s))
                    _same(view.search_grouped(q[:nq], k, s, grouping, reweighted=True), want_adj, nq, (id_base, "view grouped", k, s))
        finally:
            grouping.close()
    finally:
        view.close()


@pytest.mark.parametrize("id_base", BASES)
def test_grouped_search_with_an_id_base(oracle, id_base):
    corpus, levels, q, index, s_all, i_all = _based(id_base, oracle)
    pa, pb = np.arange(2000, 2100, 2), np.arange(2001, 2100, 2)
    for name, group_of in (("blocks", ROWS4 // 50), ("scattered", (ROWS4 * 2654435761) % 37)):
        assert ((group_of[pa] == group_of[pb]).all() if name == "blocks" else (group_of[pa] != group_of[pb]).all())
        rk = Ranking(s_all, i_all, group_of, id_base=id_base)
        grouping = index.grouping(group_of)
        try:
            for k, s in ((10, 1), (10, 3), (1, 128)):
                want_raw, want_adj = expected(oracle, rk, levels, k, s, id_base=id_base)
                assert want_raw[1].min() >= -1 and (want_raw[1][want_raw[1] >= 0] >= id_base).all()
                assert _bits(want_raw[3][want_raw[1] >= 0]) == _bits(group_of[want_raw[1][want_raw[1] >= 0] - id_base].astype(np.int32))
                for nq in (NQ4, 1, 4, 17):
                    _same(index.search_grouped(q[:nq], k, s, grouping, reweighted=False), want_raw, nq, (id_base, name, "raw", k, s))
                    _same(index.search_grouped(q[:nq], k, s, grouping, reweighted=True), want_adj, nq, (id_base, name, k, s))
        finally:
            grouping.close()


HY_RANKERS = [("rrf", {"c": 60.0}, {"ranker": "rrf", "rrf_c": 60.0}),
              ("weighted", {"weights": [0.3, 1.0, 0.7], "norm": "cosine"}, {"ranker": "weighted", "weights": [0.3, 1.0, 0.7], "norm": "cosine"})]


@pytest.mark.parametrize("id_base", BASES)
def test_hybrid_search_and_fuse_lists_with_an_id_base(oracle, id_base):
    corpus, levels, pool, index, s_all, i_all = _based(id_base, oracle)
    R, limits = 3, [10, 40, 128]
    fusion = index.fusion(256)
    mk = _Masks(index)
    try:
        for nq in (1, 17, 40):                                   # 3 / 51 / 120 sub-searches: single launch or streaming | streaming | MFMA
            sel = np.array([[20 + 3 * (qi % 20) + r for r in range(R)] for qi in range(nq)])
            sel[::5, 0] = np.arange(nq)[::5] % 20                # some requests ARE duplicated rows: equal sub-scores
            sels = [[None if (qi + r) % 3 == 0 else ROWS4 % 5 == (qi + r) % 5 for r in range(R)] for qi in range(nq)]
            dmasks = [[mk(m) for m in row] for row in sels]
            lo = np.full((nq, R), -np.inf, np.float32)
            hi = np.full((nq, R), np.inf, np.float32)
            lo[:, 1] = s_all[sel[:, 1], 25]
            hi[:, 2] = s_all[sel[:, 2], 3]
            qv = np.ascontiguousarray(pool[sel])
            for k in (10, 128):
                for ranker, okw, kw in HY_RANKERS:
                    for what, oextra, extra in (("plain", {}, {}), ("masks", {"masks": sels}, {"masks": dmasks}),
                                                ("bands", {"radius": lo, "range_filter": hi}, {"radius": lo, "range_filter": hi}),
                                                ("masks + bands", {"masks": sels, "radius": lo, "range_filter": hi}, {"masks": dmasks, "radius": lo, "range_filter": hi})):
                        want = hybrid_batch(s_all, i_all, levels, sel, limits, k, ranker, id_base=id_base, **okw, **oextra)
                        valid = want[0][1] >= 0
                        assert valid[:, 0].all() and (want[0][1][valid] >= id_base).all() and (want[0][1][valid] < id_base + N4).all()
                        if "bands" in what:   # request 1's list is cut short by its floor: its bit is set on at most 25 hits
                            assert (((want[0][3] >> 1) & 1).sum(1) <= 25).all()
                        _same(index.search_hybrid(qv, limits, k, fusion, reweighted=False, **kw, **extra), want[0], nq, (id_base, what, ranker, "raw", k, nq))
                        _same(index.search_hybrid(qv, limits, k, fusion, reweighted=True, **kw, **extra), want[1], nq, (id_base, what, ranker, k, nq))
            mk.close()
        # fuse_lists: ids below id_base and at or above id_base + n are skipped like padding (and keep their slot: rank = slot)
        nq = 17
        sel = np.array([[20 + 3 * (qi % 20) + r for r in range(R)] for qi in range(nq)])
        sc = np.ascontiguousarray(s_all[sel][:, :, :128])
        ids = np.ascontiguousarray(i_all[sel][:, :, :128])
        ids[:, :, 1] = id_base - 1
        ids[:, 1, 3] = id_base + N4
        ids[:, 2, 5] = 5                                         # a small id: below both bases
        ids[:, 0, 7] = -1
        ids[:, 2, 9] = id_base + N4 + 2**33
        for k in (10, 128):
            for ranker, okw, kw in HY_RANKERS:
                per_q = [fuse_query([(sc[qi, r, :limits[r]], ids[qi, r, :limits[r]]) for r in range(R)], levels, k, ranker, id_base=id_base, n=N4, **okw)
                         for qi in range(nq)]
                want = (tuple(np.stack([p[0][j] for p in per_q]) for j in range(4)), tuple(np.stack([p[1][j] for p in per_q]) for j in range(5)))
                valid = want[0][1] >= 0
                assert (want[0][1][valid] >= id_base).all() and (want[0][1][valid] < id_base + N4).all()
                assert not np.isin(want[0][1], [id_base - 1, id_base + N4, 5]).any()
                _same(index.fuse_lists(fusion, sc, ids, limits, k, reweighted=False, to_host=True, **kw), want[0], nq, (id_base, "fuse_lists raw", ranker, k))
                _same(index.fuse_lists(fusion, sc, ids, limits, k, reweighted=True, to_host=True, **kw), want[1], nq, (id_base, "fuse_lists", ranker, k))
    finally:
        mk.close()
        fusion.close()


# ---- 5. degenerate scores -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,nq", [(10, 1), (32, 9), (64, 65), (128, 5)])
def test_all_scores_tied_pages_are_the_rows_in_order(oracle, k, nq):
    """all-zero queries: every score is +0.0 and the cursor's (order == cursor order) & (~row < ~cursor row) term decides every row;
    a list's tie path runs at every width. k = 10 / one query: the single-launch form; 32 / 9: a pass of eight and a pass of one;
    64 / 65: the MFMA form; 128 / 5: the QB = 8 streaming form."""
    id_base = BASES[0]
    corpus, levels, _q, index, _s, _i = _based(id_base, oracle)
    zero = np.zeros((nq, 768), np.float32)
    zs, zi = oracle.flat_ip_topk(corpus, zero[:1], N4, id_base=id_base)
    assert _bits(zs) == _bits(np.zeros((1, N4), np.float32)) and (zi[0] == id_base + ROWS4).all()   # +0.0, never -0.0: id order
    want_pages = pages(zs[0], zi[0], k)
    assert [i for p in want_pages for i in p] == (id_base + ROWS4).tolist() and len(want_pages) == -(-N4 // k)
    after, got = None, []
    for p, wp in enumerate(want_pages):
        raw, ids, lv = index.search_range(zero, k, after=after, reweighted=False)
        m = len(wp)
        assert (ids == ids[0]).all() and ids[0, :m].tolist() == wp and (ids[0, m:] == -1).all(), (k, p)
        assert _bits(raw[:, :m]) == _bits(np.zeros((nq, m), np.float32)) and np.isneginf(raw[:, m:]).all()
        assert _bits(lv[0, :m]) == _bits(levels[np.array(wp) - id_base]) and (lv[:, m:] == 0).all()
        got += ids[0, :m].tolist()
        after = (raw[:, m - 1].copy(), ids[:, m - 1].copy())
    assert got == (id_base + ROWS4).tolist()                     # no row twice, none missing, in order
    raw, ids, lv = index.search_range(zero, k, after=after, reweighted=False)
    assert (ids == -1).all() and np.isneginf(raw).all() and (lv == 0).all()   # behind the last row: nothing


SUBNORMAL_SCALE = 3e-38


def test_subnormal_scores_against_subnormal_bounds(oracle):
    """the corpus scaled by 3e-38 (tests/test_gpu_parity.py::test_tiny_and_huge_norms_stay_exact): every score and therefore every
    floor, ceiling and cursor taken from the ranking behind rank 1 is subnormal. Scale 3e-38 keeps at least 100 distinct score values per
    query (asserted below; measured on the oracle: 2 990 or more of 3 000), so no other scale was needed."""
    corpus0, levels, q = _corpus4()
    corpus = np.ascontiguousarray(corpus0 * np.float32(SUBNORMAL_SCALE))
    s_all, i_all = oracle.flat_ip_topk(corpus, q, N4)
    tiny = np.finfo(np.float32).tiny
    assert (np.abs(s_all[:, 2:]) < tiny).all() and (s_all != 0).any(1).all()   # (all but a query's own row and its twin: 1.0 * 3e-38)
    distinct = np.array([len(np.unique(s_all[r].view(np.uint32))) for r in range(NQ4)])
    print(f"distinct subnormal score values per query: min {distinct.min()}")
    assert (distinct >= 100).all()
    index = IcdIndex(corpus, levels, max_nq=128, max_k=128)
    try:
        cases = {"floor": {"radius": s_all[:, 40].copy()}, "ceiling": {"range_filter": s_all[:, 200].copy()},
                 "both": {"radius": s_all[:, 230].copy(), "range_filter": s_all[:, 200].copy()},
                 "cursor": {"after": (s_all[:, 150].copy(), i_all[:, 150].copy()), "radius": s_all[:, 400].copy()}}
        assert (s_all[:, 230] < s_all[:, 200]).all()
        for name, bounds in cases.items():
            for k in (10, 32, 64, 128):
                want = band_batch(s_all, i_all, levels, k, **bounds)
                n_hits = (want[0][1] >= 0).sum(1)
                if name == "floor":
                    assert (n_hits <= min(k, 40)).all() and (n_hits == min(k, 40)).mean() > 0.8
                elif name == "ceiling":
                    assert (n_hits == k).all() and (np.abs(want[0][0]) < tiny).all()
                elif name == "both":
                    assert (n_hits >= 1).all() and (n_hits <= 32).all()   # (ranks 200 .. 229, and a tie at either end)
                else:
                    assert (want[0][1][:, 0] == i_all[:, 151]).all() and (n_hits == k).all()
                for nq in (1, 4, 9, 65, NQ4):
                    _banded(index, q, want, k, nq, ("subnormal", name), **bounds)
    finally:
        index.close()


def test_band_over_a_corpus_with_nan_and_out_of_fp16_range_components(oracle):
    """the corpus of tests/test_gpu_parity.py::test_unnormalised_and_nonfinite_inputs: a 7e4 component and a NaN one. The row whose
    score is NaN is never a hit, with or without a bound"""
    rng = np.random.default_rng(70)
    n = 2000
    corpus = (rng.standard_normal((n, 768)) * rng.uniform(0.1, 30, (n, 1))).astype(np.float32)
    levels = icd_levels(n, 71)
    q = (rng.standard_normal((70, 768)) * 5).astype(np.float32)
    corpus[17, 5] = 7e4
    corpus[18, 6] = np.nan
    s_full, i_full = oracle.flat_ip_topk(corpus, q, n)
    assert (i_full[:, -1] == -1).all() and not (i_full == 18).any() and (i_full[:, :-1] >= 0).all()   # the NaN row is in no ranking
    s_all, i_all = np.ascontiguousarray(s_full[:, :-1]), np.ascontiguousarray(i_full[:, :-1])
    assert np.isfinite(s_all).all()
    index = IcdIndex(corpus, levels, max_nq=128, max_k=128)
    nan_only = index.rowmask(np.array([18]))
    try:
        assert index.stats()["fast_path"] == 0
        for k in (10, 33, 128):
            for nq in (1, 4, 9, 65, 70):   # no bound: the band IS the MODE_EXACT search
                ps, pi = index.search(q[:nq], k, MODE_EXACT)
                g = index.search_range(q[:nq], k, reweighted=False)
                assert _bits(g[0]) == _bits(ps) and _bits(g[1]) == _bits(pi) and _bits(ps) == _bits(s_all[:nq, :k]) and _bits(pi) == _bits(i_all[:nq, :k])
            cases = {"floor": {"radius": s_all[:, 30].copy()}, "ceiling": {"range_filter": s_all[:, 200].copy()},
                     "the whole line": {"radius": np.float32(-np.inf), "range_filter": np.float32(np.inf)},
                     "behind the best hit": {"after": (s_all[:, 0].copy(), i_all[:, 0].copy()), "range_filter": s_all[:, 0].copy()},
                     "the tail": {"after": (s_all[:, n - 12].copy(), i_all[:, n - 12].copy())}}
            for name, bounds in cases.items():
                want = band_batch(s_all, i_all, levels, k, **bounds)
                assert not (want[0][1] == 18).any()
                if name == "the tail":   # ten rows are ranked behind the cursor; the NaN row is not an eleventh
                    assert ((want[0][1] >= 0).sum(1) == min(k, 10)).all()
                for nq in (1, 4, 9, 65, 70):
                    _banded(index, q, want, k, nq, ("nan corpus", name), **bounds)
            # a mask of the NaN row alone: all padding
            want = masked_batch(s_all, i_all, levels, [np.arange(n) == 18] * 70, k)
            assert (want[0][1] == -1).all()
            for nq in (1, 9, 65):
                _banded(index, q, want, k, nq, ("nan corpus", "mask of the NaN row"), masks=[nan_only] * 70)
    finally:
        nan_only.close()
        index.close()
