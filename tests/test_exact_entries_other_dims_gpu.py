"""Grouped, scored, MAX_SIM, hybrid, boosted, wide, recommend, rank-of and by-rows search at OTHER DIMS than the 32 and 768 their own
modules test them at (run with -m gpu on an MI355X): dims 96, 256, 1024, 2048 and 4096 on the data of
tests/test_exact_family_shapes_gpu.py::test_band_and_mask_at_other_dims (2 500 unit rows, 700 at dim 4096; rows 500 .. 559 are
bit-identical twin pairs; 70 queries of which 0 .. 9 ARE twin rows; id_base = 2^32 + 1 at dims 256 and 2048). The oracle's FULL
ranking - oracle.flat_ip_topk(x, q, n, id_base=...) - is computed once per dim, shared by every test of the module and never changed.
Every comparison is byte for byte over every output array, dtype and shape included, against the numpy oracles of the entry points'
own modules; the one exception is hybrid's weighted / atan ranker, within 1e-12 of the oracle as in
tests/test_hybrid_search_gpu.py::test_weighted_atan_within_1e_12_of_the_oracle. Every case asserts its own precondition on the
oracle's side before the device is touched. DESIGN.md section 29 maps the kernel instantiations to the cases here.

What each dim selects (nks = dim / 32 K-stages of the two-buffer LDS ring, cur = ks & 1):

  the three fp32-MFMA sweep copies - group_scores_kernel (grouped max / sum / avg, MAX_SIM, hybrid grouped), wide_scores_kernel (wide,
  recommend) and rankof_sweep_kernel (rank-of) - at every batch size:
      96: nks = 3, odd: a tile's last stage sits in buffer 0 | 256: nks = 8 | 1024: nks = 32, the production dim | 2048: nks = 64 |
      4096: nks = 128. Row tiles: 20 (n = 2 500: a last tile of 68 rows), 6 at dim 4096 (60 rows); query tiles: one (1 .. 70 queries;
      63 list vectors; up to 101 example vectors of a recommend call). On this data every sweep work-group owns ONE row tile - always
      so in group_scores_kernel, and by rk_plan in the two looping kernels - so the parametrised cases cover the K ring INSIDE a tile
      only. The step from a tile whose last stage sat in buffer 0 to the next tile, which refills buffer 0 first, is covered for
      wide_scores_kernel (wide, recommend) and rankof_sweep_kernel by test_two_tiles_per_work_group_at_dim_96: 40 000 rows at dim 96,
      two tiles to a work-group.
  boosted, hybrid (its banded / masked sub-searches) and by-rows (the masked kernels at k + 1), by sub-search count nq:
      nq <= 4 at a list width of 16 (k <= 16): the single-launch streaming kernel where plan_stream_one has a plan for the dim,
      else the general streaming form; a host caller's ONE query travels in the kernel arguments at dims 96 and 256 (<= 768 floats)
      and is copied at 1024 and above.
      nq <= 64: launch_stream<KP, E, QB>, QB lowered by stream_fits as dim grows - KP 16 / 32 (k 10, 16, 17): QB = 8 up to dim 2048
      (where 8 queries fill the 96 KB beside the ring exactly), 4 at 4096; KP 128 (k 128; hybrid's limits of 128; by-rows at
      k 127): 8 up to 1024, 4 at 2048 and 4096.
      nq >= 65: the fp32-MFMA exact kernel (exact_topk<KP, ..., BAND[, MASK, BOOST]>), nks as above.
  recommend_examples_kernel and byrows_gather_kernel stride dim / 4 float4s over 256 threads: one trip up to dim 1024, two at 2048,
      four at 4096 - where average_vector's target (fp32 sums in list order, one correctly rounded divide) is compared bit for bit.
  br_layout, rk_layout and the recommend / wide layouts scale with dim: dim 4096 is the largest an index takes.

Grids (thinned from the full cross product so that a case stays within twice its yardstick, test_band_and_mask_at_other_dims[dim];
every route switch above keeps a case): grouped max - four groupings x (k, group_size) (10, 1) (10, 2) (64, 1) (128, 1) (1, 128) x nq
1, 4, 40, 65, 70, raw and reweighted, device tensors at nq 4 and 70. Scorers - sum and avg x k 1, 10, the number of groups (capped by
k * group_size <= 128) x nq 1, 5, 70. MAX_SIM - lists of 1, 3, 9, a twin list, 9 .. 2; sum and mean; k 1, 10; matches on and off; one
call and a preparation of (4 lists, 64 vectors) that splits it. Hybrid - two requests, rrf and weighted / atan, limits (5, 3) and
(128, 128), plain and one masked request + one radius, nq 1 (single launch at limits (5, 3)), 4 (8 sub-searches: streaming), 65
(130: MFMA); the grouped form at limits (5, 3) / (k, group_size) (5, 3) and (128, 128) / (10, 1), rrf at nq 1, 4, 65 and weighted / atan
on queries 10 .. 26 at both. Boosted - nq 1, 2, 4, 8, 40, 64, 65, 70 x k 10, 16, 17, 128, a band and a cursor at nq 1, 4, 40, 70. Wide - k 129,
1 025 (where the workspace holds it), n + 5; first 100 / k 400; a mask mix; a band; nq 1 and 70. Recommend - three strategies x twelve
requests (P / N (1, 0) (3, 2) (16, 0) (8, 8) x stored / vectors / mixed) x k 10, 300; a mask and a band. Rank-of - nt 1, 16 x nq 1, 70, a
mask; a NaN-scored row at dim 1024. By-rows - nq 5, 70 x k 10, 127 (128 with include_self), a mask."""
import numpy as np
import pytest

import boost_oracle as bo
import byrows_oracle as bro
import grouped_hybrid_oracle as gho
import rankof_oracle as rko
import recommend_oracle as rco
import wide_oracle as wo
from conftest import icd_levels, unit_rows
from group_scorer_oracle import expected as scorer_expected
from grouped_oracle import Ranking, expected as grouped_expected
from hybrid_oracle import hybrid_batch
from maxsim_oracle import expected as maxsim_expected
from test_boosted_search_gpu import Masks, _check as boosted_check
from test_exact_family_shapes_gpu import DIM_NQ, _cut, _dim_setup
from test_group_scorer_gpu import _check as scorer_check

pytestmark = pytest.mark.gpu

from rag_project_icd10_amd import _native  # noqa: E402
from rag_project_icd10_amd._native import MODE_EXACT, IcdIndex  # noqa: E402

F = np.float32
DIMS = [96, 256, 1024, 2048, 4096]
BASE = 2**32 + 1
ID_BASE = {96: 0, 256: BASE, 1024: 0, 2048: BASE, 4096: 0}
PAIR = np.arange(10)                                   # queries 0 .. 9 ARE rows 500 + 2 j, whose twin is row 501 + 2 j


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _bits(a):
    return np.ascontiguousarray(_np(a)).tobytes()


def _eq(got, want, nq, what):
    """every output array of a call against the first nq entries of the oracle's: dtype, shape and bytes"""
    assert len(got) == len(want), what
    for j, (g, w) in enumerate(zip(got, want)):
        g, w = _np(g), np.asarray(w)[:nq]
        if g.dtype == np.int32 and w.dtype == np.uint32:   # (request bits come back as an int32 tensor from the device)
            g = g.view(np.uint32)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, j, g.dtype, w.dtype, g.shape, w.shape)
        assert _bits(g) == _bits(w), (what, "array", j, "nq", nq, "entries", np.nonzero((g != w).reshape(len(g), -1).any(1))[0][:5])


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class World:
    """one dim: _dim_setup's corpus, queries and full ranking (tests/test_exact_family_shapes_gpu.py) with an id_base, its index, and the oracle's full
    ranking of the 70 queries - computed once, shared by the module, never written to"""

    def __init__(self, dim, oracle):
        self.oracle, self.dim, self.id_base = oracle, dim, ID_BASE[dim]
        self.x, self.levels, self.q, self.s, self.i = _dim_setup(dim, oracle, self.id_base)
        n = self.n = len(self.x)
        for a in (self.x, self.levels, self.s, self.i):
            a.setflags(write=False)
        self.rows = np.arange(n, dtype=np.int64)
        self.by_row = bo.by_row(self.s, self.i, n, self.id_base)
        self.index = IcdIndex(self.x, self.levels, max_nq=256, max_k=128, id_base=self.id_base)
        self.mk = Masks(self.index)
        self._scores, self._own = {}, None
        # the twins tie bitwise and rank 0 / 1 for queries 0 .. 9, at every dim
        assert (self.i[PAIR, 0] == self.id_base + 500 + 2 * PAIR).all() and (self.i[PAIR, 1] == self.id_base + 501 + 2 * PAIR).all()
        assert _bits(self.s[PAIR, 0]) == _bits(self.s[PAIR, 1]) and (self.s[PAIR, 1] > self.s[PAIR, 2]).all()
        assert self.i.min() == self.id_base and self.i.max() == self.id_base + n - 1

    def scores(self, vector, corpus):
        """the canonical scores of one vector by row (oracle.scores), kept per vector"""
        key = np.asarray(vector, F).tobytes()
        if key not in self._scores:
            self._scores[key] = self.oracle.scores(np.asarray(vector, F), corpus)
        return self._scores[key]

    def own(self):
        """70 stored rows as queries - rows 500 .. 519 (both twins of ten pairs), then 50 drawn rows - and their full rankings: a
        twin pair shares the ranking of its query among 0 .. 9, the drawn rows are ranked here, once"""
        if self._own is None:
            drawn = np.random.default_rng(7 * self.dim).choice(self.n, 50, replace=False)
            fs, fi = self.oracle.flat_ip_topk(self.x, np.ascontiguousarray(self.x[drawn]), self.n, id_base=self.id_base)
            half = np.arange(20) // 2
            self._own = (np.concatenate([500 + np.arange(20), drawn]).astype(np.int64) + self.id_base,
                         np.concatenate([self.s[half], fs]), np.concatenate([self.i[half], fi]))
        return self._own

    def close(self):
        self.mk.close()
        self.index.close()


@pytest.fixture(scope="module")
def worlds(oracle):
    made = {}

    def get(dim):
        if dim not in made:
            made[dim] = World(dim, oracle)
        return made[dim]
    yield get
    for w in made.values():
        w.close()


def _groupings(n):
    """23 hashed groups (tests/test_search_entry_contract_gpu.py) | one group per row | a twin pair shares its group | a twin pair
    straddles two"""
    rows = np.arange(n, dtype=np.int64)
    out = {"hashed": rows * 2654435761 % 23, "own": rows.copy(), "together": rows // 2, "split": rows % 37}
    a, b = np.arange(500, 560, 2), np.arange(501, 560, 2)
    assert (out["together"][a] == out["together"][b]).all()
    assert all((out[name][a] != out[name][b]).all() for name in ("hashed", "own", "split"))
    return out


# ---- 1. grouped search, max scorer: group_scores_kernel ------------------------------------------------------------------------
GROUPED_KS = ((10, 1), (10, 2), (64, 1), (128, 1), (1, 128))   # (128, 1) and (1, 128): the largest k and group_size (k * group_size <= 128)


@pytest.mark.parametrize("dim", DIMS)
def test_grouped_search_max_scorer(worlds, dim):
    w = worlds(dim)
    first, second = w.id_base + 500 + 2 * PAIR, w.id_base + 501 + 2 * PAIR
    for name, group_of in _groupings(w.n).items():
        rk = Ranking(w.s, w.i, group_of, id_base=w.id_base)
        grouping = w.index.grouping(group_of)
        try:
            for k, s in GROUPED_KS:
                want = grouped_expected(w.oracle, rk, w.levels, k, s, id_base=w.id_base)
                ids = want[0][1]
                assert (ids[PAIR, 0] == first).all()
                if name == "together" and s >= 2:       # the twins are the two best rows of ONE group
                    assert (ids[PAIR, 1] == second).all() and (want[0][3][PAIR, 0] == want[0][3][PAIR, 1]).all()
                elif name == "together":                # ... of which one row shows
                    assert not (ids[PAIR] == second[:, None]).any()
                elif k >= 2:                            # two groups tie by their best rows: the lower id's group first
                    at = 1 if name == "own" else s         # (a group's rows stand back to back: a group of one row takes one slot)
                    assert (ids[PAIR, at] == second).all() and _bits(want[0][0][PAIR, 0]) == _bits(want[0][0][PAIR, at])
                if name == "hashed" and k * s == 128 and k > 23:
                    assert (ids[:, 23 * s:] == -1).all() and (ids[:, :23 * s] >= 0).all()      # fewer groups than k: padding
                for nq in (1, 4, 40, 65, 70):
                    for dev in ((False, True) if nq in (4, 70) else (False,)):
                        qs = _cut(w.q, nq, dev)
                        _eq(w.index.search_grouped(qs, k, s, grouping, reweighted=False), want[0], nq, (dim, name, k, s, "raw", dev))
                        _eq(w.index.search_grouped(qs, k, s, grouping, reweighted=True), want[1], nq, (dim, name, k, s, "reweighted", dev))
        finally:
            grouping.close()


# ---- 2. sum and avg scorers: group_scores_kernel, then group_aggregate_kernel -----------------------------------------------------
@pytest.mark.parametrize("dim", DIMS)
def test_grouped_search_sum_and_avg_scorers(worlds, dim):
    w = worlds(dim)
    for name, group_of in _groupings(w.n).items():
        rk = Ranking(w.s, w.i, group_of, id_base=w.id_base)
        groups = len(np.unique(group_of))
        grouping = w.index.grouping(group_of)
        try:
            grouping.prepare_scorers(w.index)
            for k, s in ((1, 3), (10, 3), (min(groups, 128 // 3), 3)):
                for scorer in ("sum", "avg"):
                    want = scorer_expected(w.oracle, rk, w.levels, k, s, scorer, id_base=w.id_base)
                    gsc, gid = want[2]
                    assert (gid >= 0).all() and np.isfinite(gsc).all()                       # k groups rank for every query
                    if name == "together":   # the twins' group leads under both scorers: its two best rows score what no other row does
                        assert (gid[PAIR, 0] == 250 + PAIR).all() and (want[0][1][PAIR, 1] == w.id_base + 501 + 2 * PAIR).all()
                    if k == groups:          # every group is a winner: the order is the scorer's alone
                        assert all(sorted(gid[r].tolist()) == sorted(np.unique(group_of).tolist()) for r in (0, 69))
                    for nq in (1, 5, 70):
                        scorer_check(w.index, grouping, w.q[:nq], want, k, s, scorer, (dim, name, k, s, scorer, nq))
        finally:
            grouping.close()


# ---- 3. MAX_SIM: group_scores_kernel, then maxsim_kernel ---------------------------------------------------------------------------
# the vectors of the lists, as query numbers: 1, 3 and 9 vectors; a list holding a twin query pair (query 0 twice: the same bits)
# and a second twin row; then 9, 9, 9, 9, 9 and 2
LIST_VECTORS = list(range(10, 23)) + [0, 0, 1] + list(range(23, 70))
LIST_SIZES = [1, 3, 9, 3, 9, 9, 9, 9, 9, 2]
TWIN_LIST = 3


@pytest.mark.parametrize("dim", DIMS)
def test_embedding_lists_max_sim(worlds, dim):
    w = worlds(dim)
    vec = np.array(LIST_VECTORS)
    off = np.concatenate([[0], np.cumsum(LIST_SIZES)]).astype(np.int64)
    assert off[-1] == len(vec) == 63
    qv = np.ascontiguousarray(w.q[vec])
    dq = _dev(qv)
    gs = _groupings(w.n)
    for name in ("hashed", "own", "together"):
        group_of = gs[name]
        rk = Ranking(w.s[vec], w.i[vec], group_of, id_base=w.id_base)
        whole, split = w.index.grouping(group_of), w.index.grouping(group_of)
        try:
            whole.prepare_maxsim(w.index, 16, 128)      # the batch in ONE call
            split.prepare_maxsim(w.index, 4, 64)        # smaller than the batch: calls of 4 lists (16 vectors), 4 (36) and 2 (11)
            for scorer in ("sum", "mean"):
                for k in (1, 10):
                    want = maxsim_expected(rk, off, w.levels, k, scorer, id_base=w.id_base)
                    assert (want[1] >= 0).all()
                    if name == "own" and k == 10:       # rows 500 and 501 tie under every vector of the twin list: the lower row first
                        assert want[1][TWIN_LIST, :2].tolist() == [500, 501] and _bits(want[0][TWIN_LIST, 0]) == _bits(want[0][TWIN_LIST, 1])
                        t0 = int(off[TWIN_LIST])
                        assert _bits(want[2][t0]) == _bits(want[2][t0 + 1]) and _bits(want[3][t0]) == _bits(want[3][t0 + 1])
                    what = (dim, name, scorer, k)
                    _eq(w.index.search_lists(qv, off, k, whole, scorer=scorer), want, len(vec), what + ("host",))
                    _eq(w.index.search_lists(qv, off, k, split, scorer=scorer), want, len(vec), what + ("split",))
                    _eq(w.index.search_lists(qv, off, k, whole, scorer=scorer, matches=False), want[:2], len(vec), what + ("no matches",))
                    if k == 10:
                        _eq(w.index.search_lists(dq, off, k, whole, scorer=scorer), want, len(vec), what + ("device",))
            assert split.maxsim == (4, 64)
        finally:
            whole.close()
            split.close()


# ---- 4. hybrid and hybrid grouped: the banded / masked kernels per request, then hybrid_fuse.hpp -----------------------------------
ATAN_W = [0.3, 1.0]
# queries of 10 .. 26 the oracle leaves clear for the by-id comparison of the grouped atan case, the least over the five dims (measured
# on the oracle on the CPU; per dim 96 / 256 / 1024 / 2048 / 4096: hashed at limits (5, 3) 13 / 15 / 16 / 14 / 14, at (128, 128)
# 9 / 14 / 15 / 13 / 13; together at (5, 3) 14 / 16 / 16 / 15 / 16, at (128, 128) 17 at every dim)
GROUPED_ATAN_FLOOR = {("hashed", 5): 13, ("hashed", 128): 9, ("together", 5): 14, ("together", 128): 17}


def _hybrid_sel(nq):
    """request 0 is query qi; request 1 the same query for every third (full overlap), else another one"""
    qi = np.arange(nq)
    return np.stack([qi, np.where(qi % 3 == 0, qi, (qi + 11) % DIM_NQ)], axis=1)


def _atan_close(got, want, what):
    """the device's atan need not round as the host's does: fused scores within 1e-12 absolute; ids wherever the oracle's neighbouring
    fused scores differ by more than 1e-9 (tests/test_hybrid_search_gpu.py::test_weighted_atan_within_1e_12_of_the_oracle)"""
    fused, ids, lv, bits = (_np(g) for g in got)
    wf, wi, wl, wb = want
    nq = len(wf)
    valid = wi >= 0
    assert np.array_equal(ids >= 0, valid), what
    err = np.abs(fused[valid] - wf[valid]).max()
    print(f"atan {what}: max |fused - oracle| = {err:.3e}")
    assert err <= 1e-12, what
    gap_prev = np.concatenate([np.full((nq, 1), np.inf), np.abs(np.diff(wf, axis=1))], axis=1)
    gap_next = np.concatenate([np.abs(np.diff(wf, axis=1)), np.full((nq, 1), np.inf)], axis=1)
    clear = valid & (np.nan_to_num(gap_prev, nan=np.inf) > 1e-9) & (np.nan_to_num(gap_next, nan=np.inf) > 1e-9)
    assert np.array_equal(ids[clear], wi[clear]) and np.array_equal(lv[clear], wl[clear]) and np.array_equal(bits[clear], wb[clear]), what
    return int(clear.sum()), int(valid.sum())


def _atan_close_grouped(got, want, clear, id_base, what):
    """the grouped form (tests/test_hybrid_grouped_gpu.py::test_weighted_atan_within_1e_12_of_the_oracle): fused and adjusted scores
    within 1e-12; ids, levels, bits and groups for every query whose fused heads are pairwise more than 1e-9 apart"""
    valid = want[2] >= 0
    for j in (2, 3, 4, 5):
        x = want[j][clear].astype(np.int64)
        if j == 2:
            x = np.where(x >= 0, x + id_base, -1)
        assert np.array_equal(_np(got[j])[clear].astype(np.int64), x), (what, j)
    for j in (0, 1):
        err = np.abs(_np(got[j])[clear][valid[clear]] - want[j][clear][valid[clear]]).max()
        print(f"atan {what}: max |{('adj', 'fused')[j]} - oracle| = {err:.3e}")
        assert err <= 1e-12, (what, j)


@pytest.mark.parametrize("dim", DIMS)
def test_hybrid_search(worlds, dim):
    w = worlds(dim)
    fusion = w.index.fusion(256)
    third = w.rows % 3 == 1
    try:
        compared = total = 0
        for nq in (1, 4, 65):                               # 2 / 8 / 130 sub-searches
            sel = _hybrid_sel(nq)
            qv = np.ascontiguousarray(w.q[sel])
            sels = [[third, None] for _ in range(nq)]          # request 0 masked ...
            dmasks = [[w.mk(third), None] for _ in range(nq)]
            lo = np.full((nq, 2), -np.inf, F)
            lo[:, 1] = w.s[sel[:, 1], 40]                      # ... request 1 under a floor at its rank-40 score
            for limits, k in (([5, 3], 10), ([128, 128], 128)):
                for what, okw, kw in (("plain", {}, {"mode": MODE_EXACT}), ("mask + radius", {"masks": sels, "radius": lo}, {"masks": dmasks, "radius": lo})):
                    want = hybrid_batch(w.s, w.i, w.levels, sel, limits, k, "rrf", c=60.0, id_base=w.id_base, **okw)
                    ids = want[0][1]
                    assert (ids[:, 0] >= w.id_base).all()
                    if what == "plain":
                        assert ((ids >= 0).sum(1) <= sum(limits)).all() and ((want[0][3] == 3).sum(1) >= np.where(sel[:, 0] == sel[:, 1], min(limits), 0)).all()
                        if limits[0] == 128:                 # query 0's twins lead both lists, ranks 0 and 1
                            assert ids[0, :2].tolist() == [w.id_base + 500, w.id_base + 501] and want[0][0][0, 0] > want[0][0][0, 1]
                    else:                                    # request 0's hits lie inside its mask, request 1's list is cut by its floor
                        r0 = (want[0][3] & 1) == 1
                        assert third[ids[r0] - w.id_base].all() and (((want[0][3] >> 1) & 1).sum(1) <= 40).all()
                    _eq(w.index.search_hybrid(qv, limits, k, fusion, ranker="rrf", rrf_c=60.0, reweighted=False, **kw), want[0], nq, (dim, what, "rrf raw", limits, nq))
                    _eq(w.index.search_hybrid(qv, limits, k, fusion, ranker="rrf", rrf_c=60.0, reweighted=True, **kw), want[1], nq, (dim, what, "rrf", limits, nq))
                    want = hybrid_batch(w.s, w.i, w.levels, sel, limits, k, "weighted", weights=ATAN_W, norm="atan", id_base=w.id_base, **okw)
                    got = w.index.search_hybrid(qv, limits, k, fusion, ranker="weighted", weights=ATAN_W, norm="atan", reweighted=False, **kw)
                    c, t = _atan_close(got, want[0], (dim, what, limits, nq))
                    compared, total = compared + c, total + t
        # a twin pair inside a list fuses to two EQUAL scores, which the 1e-9 rule leaves out. Measured on the oracle on the CPU: 97.95 %,
        # 97.76 %, 98.15 % and 98.48 % of the ranks are compared at dims 96, 256, 1024 and 2048, 94.90 % at 4096 (60 twins in 700 rows)
        print(f"atan: {compared} of {total} ranks compared by id")
        assert compared >= (0.94 if dim == 4096 else 0.97) * total
    finally:
        fusion.close()


@pytest.mark.parametrize("dim", DIMS)
def test_hybrid_search_grouped(worlds, dim):
    w = worlds(dim)
    fusion = w.index.fusion(256)
    local = w.i - w.id_base                                 # (grouped_hybrid_oracle walks rows; the ids move to id_base + row below)
    gs = _groupings(w.n)
    try:
        for name in ("hashed", "together"):
            group_of = gs[name]
            grouping = w.index.grouping(group_of.astype(np.int32))
            try:
                for limits, (k, s) in (([5, 3], (5, 3)), ([128, 128], (10, 1))):
                    sel = _hybrid_sel(65)
                    raw, adj, _ = gho.hybrid_grouped_batch(w.s, local, group_of, w.levels, sel, limits, k, s, "rrf", 60.0)
                    raw = raw[:1] + (np.where(raw[1] >= 0, raw[1] + w.id_base, -1),) + raw[2:]
                    adj = adj[:2] + (np.where(adj[2] >= 0, adj[2] + w.id_base, -1),) + adj[3:]
                    assert (raw[1][:, 0] >= w.id_base).all()
                    if name == "together" and s == 3:      # query 0: the twins are one group's two best members, fused alike
                        assert raw[1][0, :2].tolist() == [w.id_base + 500, w.id_base + 501] and raw[4][0, 0] == raw[4][0, 1] == 250
                    # weighted / atan on queries 10 .. 26 (0 .. 9 hold their own twin pair); a query is compared by id when its fused
                    # heads are pairwise more than 1e-9 apart - two listed twins of different groups fuse to EQUAL scores and take it out
                    _, a_adj, gaps = gho.hybrid_grouped_batch(w.s, local, group_of, w.levels, sel, limits, k, s, "weighted", 60.0, ATAN_W, "atan")
                    clear = gaps[10:27] > 1e-9
                    print(f"atan grouped {dim} {name} {limits}: {int(clear.sum())} of 17 queries compared by id")
                    assert clear.sum() >= GROUPED_ATAN_FLOOR[name, limits[0]]
                    for nq in (1, 4, 65):
                        qv = np.ascontiguousarray(w.q[sel[:nq]])
                        kw = dict(grouping=grouping, group_size=s)
                        _eq(w.index.search_hybrid(qv, limits, k, fusion, ranker="rrf", reweighted=False, **kw), raw, nq, (dim, name, "raw", limits, nq))
                        _eq(w.index.search_hybrid(qv, limits, k, fusion, ranker="rrf", reweighted=True, **kw), adj, nq, (dim, name, limits, nq))
                    got = w.index.search_hybrid(np.ascontiguousarray(w.q[sel[10:27]]), limits, k, fusion, ranker="weighted", weights=ATAN_W, norm="atan", **kw)
                    _atan_close_grouped(got, tuple(x[10:27] for x in a_adj), clear, w.id_base, (dim, name, limits))
            finally:
                grouping.close()
    finally:
        fusion.close()


# ---- 5. boosted search: the BOOST instantiations of the single-launch, streaming and MFMA exact kernels -------------------------------
def _tie_weight(s_row, s_twin):
    """a positive normal fp32 w with fl(s_row * w) == s_twin bit for bit, or None: the quotient and its neighbours"""
    with np.errstate(all="ignore"):
        w = F(np.float64(s_twin) / np.float64(s_row))
        for _ in range(40):
            w = np.nextafter(w, F(0))
        for _ in range(81):
            if np.isfinite(w) and w > 0 and F(s_row * w).tobytes() == F(s_twin).tobytes():
                return w
            w = np.nextafter(w, F(np.inf))
    return None


def _boost_table(w):
    """per query two slots. Slot 1 demotes (0.5) the odd rows of the twin block and every row r % 7 == 3 outside it: it breaks every
    twin pair's tie. Slot 0 promotes: queries 0 .. 9 ONE non-twin row by the weight that lifts it onto the twin's score bit for bit (a
    tie between a twin and a non-twin row, found on the oracle's scores); the others rows r % 3 == 0 by 1.5."""
    block = (w.rows >= 500) & (w.rows < 560)
    demote = (block & (w.rows % 2 == 1)) | (~block & (w.rows % 7 == 3))
    promote = w.rows % 3 == 0
    table, lifted = [], []
    for qi in range(DIM_NQ):
        if qi >= 10:
            table.append([(promote, F(1.5)), (demote, F(0.5))])
            continue
        found = None
        for rank in range(2, 60):
            row = int(w.i[qi, rank] - w.id_base)
            if block[row] or demote[row] or not w.s[qi, rank] > 0:
                continue
            wt = _tie_weight(w.s[qi, rank], w.s[qi, 0])
            if wt is not None:
                found = (row, wt)
                break
        assert found is not None, qi
        lifted.append(found[0])
        table.append([(w.rows == found[0], found[1]), (demote, F(0.5))])
    return table, lifted


@pytest.mark.parametrize("dim", DIMS)
def test_boosted_search(worlds, dim):
    w = worlds(dim)
    table, lifted = _boost_table(w)
    rk = bo.boosted_rankings(w.by_row, table, w.id_base)
    for qi in range(10):    # the even twin and the lifted row tie at the top, by id; the odd twin fell to half its score
        top = sorted([w.id_base + 500 + 2 * qi, w.id_base + lifted[qi]])
        assert rk[qi][1][:2].tolist() == top and _bits(rk[qi][0][0]) == _bits(rk[qi][0][1]) and rk[qi][0][1] > rk[qi][0][2]
        at = int(np.nonzero(rk[qi][1] == w.id_base + 501 + 2 * qi)[0][0])
        assert at >= 2 and _bits(rk[qi][0][at]) == _bits(w.s[qi, 0] * F(0.5))
    ws = w.index.boost_workspace(128)
    handles = w.mk.boosts(table)
    try:
        for k in (10, 16, 17, 128):
            want = bo.boosted_batch(w.by_row, w.levels, table, k, id_base=w.id_base, rankings=rk)
            assert (want[0][1] >= 0).all()
            for nq in (1, 2, 4, 8, 40, 64, 65, 70):
                boosted_check(w.index, ws, w.q, want, k, nq, (dim, "boosted", k), handles)
        # one band and one cursor, both on the BOOSTED score: ranks 31 .. 150 of it, and the page behind the first of the tied pair
        lo = np.array([rk[qi][0][150] for qi in range(DIM_NQ)], F)
        hi = np.array([rk[qi][0][30] for qi in range(DIM_NQ)], F)
        after = (np.array([rk[qi][0][0] for qi in range(DIM_NQ)], F), np.array([rk[qi][1][0] for qi in range(DIM_NQ)], np.int64))
        for k in (16, 128):
            band = bo.boosted_batch(w.by_row, w.levels, table, k, radius=lo, range_filter=hi, id_base=w.id_base, rankings=rk)
            assert _bits(band[0][0][:, 0]) == _bits(hi) and (band[0][0][:, min(k, 100) - 1] > lo).all()
            page = bo.boosted_batch(w.by_row, w.levels, table, k, after=after, id_base=w.id_base, rankings=rk)
            assert all(page[0][1][qi, 0] == rk[qi][1][1] for qi in range(DIM_NQ)) and _bits(page[0][0][PAIR, 0]) == _bits(after[0][PAIR])
            for nq in (1, 4, 40, 70):
                boosted_check(w.index, ws, w.q, band, k, nq, (dim, "band", k), handles, radius=lo, range_filter=hi)
                boosted_check(w.index, ws, w.q, page, k, nq, (dim, "cursor", k), handles, after=after)
    finally:
        ws.close()


# ---- 6. wide search: wide_scores_kernel -----------------------------------------------------------------------------------------
def _wide(w, ws, want, k, nq, what, first=0, sels=None, radius=None, range_filter=None):
    hm = None if sels is None else [w.mk(m) for m in sels[:nq]]
    cut = lambda v: None if v is None else v[:nq]   # noqa: E731
    for rew in (False, True):
        got = ws.search_wide(w.q[:nq], k, masks=hm, radius=cut(radius), range_filter=cut(range_filter), first=first, reweighted=rew)
        if rew:
            _eq(got[:4], want[1], nq, what + ("reweighted",))
        else:
            assert got[0] is None
            _eq(got[1:4], want[0], nq, what + ("raw",))
        _eq(got[4:], want[2:], nq, what + ("count, selected", rew))


@pytest.mark.parametrize("dim", DIMS)
def test_wide_search(worlds, dim):
    w = worlds(dim)
    n = w.n
    max_k = min(n + 5, 16384)
    ws = _native.IcdWide(w.index, DIM_NQ, max_k)
    try:
        for k in sorted({129, min(1025, max_k), n + 5}):      # (1 025 above the workspace's n + 5 at dim 4096, where n = 700)
            want = wo.wide_batch(w.s, w.i, w.levels, k, id_base=w.id_base)
            raw, _adj, count, selected = want
            assert (count == min(k, n)).all() and (selected == n).all() and (raw[1][:, min(k, n):] == -1).all()
            if k > n:
                assert np.isneginf(raw[0][:, n:]).all() and (raw[1][:, n - 1] >= 0).all()              # k beyond n pads
            assert (raw[1][PAIR, 0] == w.id_base + 500 + 2 * PAIR).all() and (raw[1][PAIR, 1] == w.id_base + 501 + 2 * PAIR).all()
            for nq in (1, DIM_NQ):
                _wide(w, ws, want, k, nq, (dim, k, nq))
        want = wo.wide_batch(w.s, w.i, w.levels, 400, first=100, id_base=w.id_base)
        assert _bits(want[0][1]) == _bits(w.i[:, 100:500]) and (want[2] == 400).all()
        for nq in (1, DIM_NQ):
            _wide(w, ws, want, 400, nq, (dim, "first", nq), first=100)
        # a per-query mask mix and a band whose bounds equal scores that occur (radius is strict, range_filter inclusive)
        half, empty = ((w.rows * 2654435761) >> 7) & 1 == 1, np.zeros(n, bool)
        sels = [(None, half, empty)[r % 3] for r in range(DIM_NQ)]
        want = wo.wide_batch(w.s, w.i, w.levels, 300, masks=sels, id_base=w.id_base)
        assert want[3].tolist() == [(n, int(half.sum()), 0)[r % 3] for r in range(DIM_NQ)] and (want[2][2::3] == 0).all() and (want[2][1::3] == 300).all()
        lo, hi = w.s[:, 450].copy(), w.s[:, 30].copy()
        banded = wo.wide_batch(w.s, w.i, w.levels, 500, radius=lo, range_filter=hi, id_base=w.id_base)
        for r in range(DIM_NQ):
            real = banded[0][0][r][banded[0][1][r] >= 0]
            assert _bits(real[0]) == _bits(hi[r]) and real[-1] > lo[r] and (w.s[r] == lo[r]).any() and 415 <= len(real) <= 425
        for nq in (1, DIM_NQ):
            _wide(w, ws, want, 300, nq, (dim, "masks", nq), sels=sels)
            _wide(w, ws, banded, 500, nq, (dim, "band", nq), radius=lo, range_filter=hi)
    finally:
        ws.close()


# ---- 7. recommend: recommend_examples_kernel, then wide_scores_kernel ------------------------------------------------------------------
RECOMMEND_SHAPES = ((1, 0), (3, 2), (16, 0), (8, 8))


def _requests(w):
    """twelve requests: every P / N shape with stored rows (the first a twin, the second its partner), with caller vectors (the
    queries, from 10 on) and with the two in turn"""
    rng = np.random.default_rng(w.dim + 1)
    reqs, v = [], 10
    for P, N in RECOMMEND_SHAPES:
        for kind in ("stored", "vector", "mixed"):
            ex = []
            for j in range(P + N):
                if kind == "stored" or (kind == "mixed" and j % 2 == 0):
                    ex.append(int((500, 501)[j] if j < 2 else rng.integers(0, w.n)) + w.id_base)
                else:
                    ex.append(w.q[v % DIM_NQ].copy())
                    v += 1
            reqs.append((ex[:P], ex[P:]))
    return reqs


def _recommend(w, ws, want, P, N, strategy, k, what, sels=None, radius=None, range_filter=None, forms=(False, True)):
    hm = None if sels is None else [w.mk(m) for m in sels]
    for rew in forms:
        got = ws.recommend(P, N, strategy, k, masks=hm, radius=radius, range_filter=range_filter, reweighted=rew)
        if rew:
            _eq(got[:4], want[1], len(P), what + ("reweighted",))
        else:
            assert got[0] is None
            _eq(got[1:4], want[0], len(P), what + ("raw",))
        _eq(got[4:], want[2:], len(P), what + ("count, selected", rew))


@pytest.mark.parametrize("dim", DIMS)
def test_recommend(worlds, dim):
    w = worlds(dim)
    n = w.n
    reqs = _requests(w)
    P, N = [r[0] for r in reqs], [r[1] for r in reqs]
    ws = _native.IcdRecommend(w.index, 16, None, 1024)
    half = ((w.rows * 2654435761) >> 7) & 1 == 1
    try:
        for strategy in rco.STRATEGIES:
            oracle = lambda k, **kw: rco.recommend_batch(w.x, w.levels, P, N, strategy, k, id_base=w.id_base, score_fn=w.scores, **kw)   # noqa: E731
            for k in (10, 300):
                want = oracle(k)
                raw, _adj, count, selected = want
                stored = np.array([len(set(rco.example_rows(p + q, w.id_base))) for p, q in reqs])
                assert (count == k).all() and (selected == n - stored).all() and stored.max() >= 8            # a request's stored examples never rank
                assert not any(set(raw[1][r].tolist()) & {e for e in reqs[r][0] + reqs[r][1] if isinstance(e, int)} for r in range(len(reqs)))
                _recommend(w, ws, want, P, N, strategy, k, (dim, strategy, k), forms=(False, True) if k == 10 else (False,))
                if strategy == "average_vector":   # the target itself: the multi-trip loop of recommend_examples_kernel at 2048 and 4096
                    target = np.stack([rco.target_vector(p, q, w.x, w.id_base) for p, q in reqs])
                    assert len({t.tobytes() for t in target}) >= len(reqs) - 1   # (row 500 alone is the target of two requests)
                    _eq([ws.last_vectors(len(reqs))], [target], len(reqs), (dim, "target vectors", k))
            full = oracle(600)[0][0]
            lo, hi = full[:, 200].copy(), full[:, 5].copy()
            assert (lo < hi).all()
            want = oracle(300, masks=[half] * len(reqs), radius=lo, range_filter=hi)
            assert (want[3] >= 40).all() and (want[3] <= 196).all() and (want[2] == want[3]).all() and half[want[0][1][want[0][1] >= 0] - w.id_base].all()
            _recommend(w, ws, want, P, N, strategy, 300, (dim, strategy, "mask + band"), sels=[half] * len(reqs), radius=lo, range_filter=hi)
    finally:
        ws.close()


# ---- 8. rank-of: rankof_sweep_kernel, mmr_quad_chain ---------------------------------------------------------------------------------
def _targets(w, nq, nt):
    """column 0: a twin row - for queries 0 .. 9 their own odd twin, rank 1 behind its partner; nt = 1: every third query row n - 1,
    every third a non-twin row instead; nt = 16: the even twin, row n - 1, row 0, drawn rows, one id outside the index, padding last"""
    qs = np.arange(nq)
    t = np.random.default_rng(w.dim + nt).integers(0, w.n, (nq, nt))
    t[:, 0] = 501 + 2 * (qs % 10)
    if nt == 1:
        t[qs % 3 == 1, 0] = w.n - 1
        t[(qs % 3 == 2) & (qs >= 10), 0] = 7
    else:
        t[:, 1], t[:, 2], t[:, 3], t[:, 4] = 500 + 2 * (qs % 10), w.n - 1, 0, w.n
    t = t + w.id_base
    if nt > 1:
        t[:, -1] = -1
    return t.astype(np.int64)


@pytest.mark.parametrize("dim", [96, 1024, 2048, 4096])
def test_rank_of(worlds, oracle, dim):
    w = worlds(dim)
    ws = _native.IcdRankOf(w.index)
    odd = (w.rows % 2 == 1) | (w.rows == 0)               # admits the odd twins, not the even ones, and row 0
    try:
        for nt in (1, 16):
            for nq in (1, DIM_NQ):
                tg = _targets(w, nq, nt)
                want = rko.rank_of_batch(w.s[:nq], w.i[:nq], w.levels, tg, None, w.n, w.id_base)
                m = min(nq, 10)
                own = np.arange(m)[(np.arange(m) % 3 != 1) | (nt > 1)]       # (the queries whose first target is their own odd twin)
                assert (want[0][own, 0] == 1).all()
                if nt > 1:
                    assert (want[0][:m, 1] == 0).all() and _bits(want[2][:m, 0]) == _bits(want[2][:m, 1])      # the twins: ranks 0 and 1, one score
                    assert (want[0][:, 4] == -1).all() and (want[0][:, -1] == -1).all() and (want[0][:, 2] >= 0).all()
                _eq(ws.rank_of(w.q[:nq], tg), want, nq, (dim, nt, nq))
                masked = rko.rank_of_batch(w.s[:nq], w.i[:nq], w.levels, tg, [odd] * nq, w.n, w.id_base)
                assert (masked[4] == odd.sum()).all()
                if nt > 1:   # the even twin is outside the mask: no rank; the odd one leads what is left
                    assert (masked[0][:m, 1] == -1).all() and (masked[0][:m, 0] == 0).all() and (masked[0][:, 3] >= 0).all()
                _eq(ws.rank_of(w.q[:nq], tg, [w.mk(odd)] * nq), masked, nq, (dim, nt, nq, "mask"))
    finally:
        ws.close()
    if dim == 1024:   # a NaN-scored row: in no ranking, rank -1 and NaN scores, its level kept
        x = w.x[:300].copy()
        x[5, dim // 2] = np.nan
        fs, fi = oracle.flat_ip_topk(x, w.q[:5], 300)
        assert (fi[:, -1] == -1).all() and not (fi == 5).any()
        index = IcdIndex(x, w.levels[:300], max_nq=8, max_k=16, probe=False)
        ws = _native.IcdRankOf(index)
        try:
            tg = np.tile(np.array([5, 6, 299, 0], np.int64), (5, 1))
            want = rko.rank_of_batch(fs, fi, w.levels[:300], tg, None, 300)
            assert (want[0][:, 0] == -1).all() and np.isnan(want[2][:, 0]).all() and (want[3][:, 0] == w.levels[5]).all() and (want[0][:, 1:] >= 0).all()
            _eq(ws.rank_of(w.q[:5], tg), want, 5, (dim, "NaN row"))
        finally:
            ws.close()
            index.close()


# ---- 8b. dim 96, more than one tile per work-group: the tile-to-tile transition of wide_scores_kernel and rankof_sweep_kernel -------------
BIG_N = 40000


def _tiles_per_work_group(n, nq):
    """rankof_plan.hpp rk_plan for this device: the row tiles one sweep work-group of wide_scores_kernel / rankof_sweep_kernel walks"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    mtiles, row_tiles = -(-nq // 128), -(-n // 128)
    want = min(row_tiles, max(1, cus // mtiles))
    return -(-row_tiles // want)


def test_two_tiles_per_work_group_at_dim_96(oracle):
    """nks = 3 is odd: a tile's last stage is read from LDS buffer 0, the buffer the NEXT tile of the same work-group refills first
    (behind the barrier at the head of the tile loop). At n = 2 500 every work-group of the two looping sweeps owns ONE tile;
    at n = 40 000 (313 tiles, the last of 64 rows) a work-group walks two (asserted from rk_plan and the device's CU count).
    wide and rank-of: 1 and 16 queries; recommend: six requests of 1 .. 16 examples (44 vectors). group_scores_kernel gives a work-group ONE tile by construction: it has no
    such transition."""
    dim, nq, id_base = 96, 16, BASE
    x = unit_rows(BIG_N, dim, 4000 + dim)
    x[501:560:2] = x[500:560:2]
    rng = np.random.default_rng(96 + BIG_N)
    q = x[rng.integers(0, BIG_N, nq - 10)] + (0.3 / np.sqrt(dim)) * rng.standard_normal((nq - 10, dim)).astype(F)
    q = np.ascontiguousarray(np.concatenate([x[500:520:2], q]), dtype=F)
    levels = icd_levels(BIG_N, dim)
    s_all, i_all = oracle.flat_ip_topk(x, q, BIG_N, id_base=id_base)
    assert (i_all[PAIR, 0] == id_base + 500 + 2 * PAIR).all() and (i_all[PAIR, 1] == id_base + 501 + 2 * PAIR).all() and _bits(s_all[PAIR, 0]) == _bits(s_all[PAIR, 1])
    assert _tiles_per_work_group(BIG_N, nq) >= 2 and _tiles_per_work_group(BIG_N, 44) >= 2
    rows = np.arange(BIG_N)
    half = ((rows * 2654435761) >> 7) & 1 == 1
    index = IcdIndex(x, levels, max_nq=256, max_k=128, id_base=id_base)
    wide, rank, rec = _native.IcdWide(index, nq, 2048), _native.IcdRankOf(index), _native.IcdRecommend(index, 16, None, 1024)
    mask = index.rowmask(np.nonzero(half)[0])
    try:
        # wide: a hit's score is a sum over all three stages of its tile, whichever tile of the work-group's it lies in
        for k, sels in ((129, None), (1025, None), (300, [half] * nq)):
            want = wo.wide_batch(s_all, i_all, levels, k, masks=sels, id_base=id_base)
            assert (want[2] == k).all() and len(np.unique((want[0][1] - id_base) // 128)) >= 200      # hits from all over the tiles
            for m in (1, nq):
                for rew in (False, True):
                    got = wide.search_wide(q[:m], k, masks=None if sels is None else [mask] * m, reweighted=rew)
                    _eq(got[:4] if rew else got[1:4], want[1] if rew else want[0], m, ("wide", k, m, rew))
                    _eq(got[4:], want[2:], m, ("wide count, selected", k, m, rew))
        # rank-of: the count runs over every tile of every chunk; targets in first and second tiles of a chunk and in the last tile
        tg = rng.integers(0, BIG_N, (nq, 16))
        tg[:, 0], tg[:, 1], tg[:, 2], tg[:, 3], tg[:, 4] = 501 + 2 * (np.arange(nq) % 10), 0, 128, 383, BIG_N - 1
        tg = (tg + id_base).astype(np.int64)
        for sels in (None, [half] * nq):
            want = rko.rank_of_batch(s_all, i_all, levels, tg, sels, BIG_N, id_base)
            if sels is None:
                assert (want[0][PAIR, 0] == 1).all() and (want[0] >= 0).all() and want[0].max() > BIG_N // 2
            for m in (1, nq):
                _eq(rank.rank_of(q[:m], tg[:m], None if sels is None else [mask] * m), want, m, ("rank-of", m, sels is not None))
        # recommend: the examples' scores come from the same sweep
        reqs, v, cache = [], 0, {}
        for P, N in ((1, 0), (3, 2), (16, 0)):
            for kind in ("stored", "mixed"):
                ex = [int(rng.integers(0, BIG_N)) + id_base if kind == "stored" or (kind == "mixed" and j % 2 == 0) else q[(v + j) % nq].copy() for j in range(P + N)]
                v += P + N
                reqs.append((ex[:P], ex[P:]))
        Ps, Ns = [r[0] for r in reqs], [r[1] for r in reqs]

        def scores(vector, corpus):
            key = np.asarray(vector, F).tobytes()
            if key not in cache:
                cache[key] = oracle.scores(np.asarray(vector, F), corpus)
            return cache[key]
        for strategy in rco.STRATEGIES:
            want = rco.recommend_batch(x, levels, Ps, Ns, strategy, 300, id_base=id_base, score_fn=scores)
            assert (want[2] == 300).all()
            got = rec.recommend(Ps, Ns, strategy, 300, reweighted=False)
            assert got[0] is None
            _eq(got[1:4], want[0], len(reqs), ("recommend", strategy))
            _eq(got[4:], want[2:], len(reqs), ("recommend count, selected", strategy))
    finally:
        for h in (mask, wide, rank, rec):
            h.close()
        index.close()


# ---- 9. by-rows: byrows_gather_kernel, then the masked kernels at k + 1 ------------------------------------------------------------------
@pytest.mark.parametrize("dim", [96, 2048, 4096])
def test_search_by_rows(worlds, dim):
    w = worlds(dim)
    ids, fs, fi = w.own()
    ws = w.index.byrows(128)
    third = w.rows % 3 != 1                                 # rows 502, 505, .. are outside: some ids lie outside their own mask
    try:
        assert (fi[:20, 0] == w.id_base + 500 + 2 * (np.arange(20) // 2)).all() and (fi[:20, 1] == fi[:20, 0] + 1).all()
        for include_self, k in ((False, 10), (False, 127), (True, 10), (True, 128)):
            for sel in (None, third):
                bools = None if sel is None else [sel] * len(ids)
                raw, rew = bro.byrows_batch(fs, fi, w.levels, ids, k, masks=bools, id_base=w.id_base, include_self=include_self)
                if sel is None and not include_self:   # no row is its own neighbour; a twin's first neighbour is its partner
                    assert (raw[1] != ids[:, None]).all() and (raw[1][:20, 0] - w.id_base == ((ids[:20] - w.id_base) ^ 1)).all()
                if sel is None and include_self:       # both twins lead every list of their pair, the lower id first
                    assert (raw[1][:20, 0] - w.id_base == ((ids[:20] - w.id_base) & ~1)).all() and (raw[1][:20, 1] == raw[1][:20, 0] + 1).all()
                if sel is not None:
                    assert ((raw[1] >= 0).sum(1) == k).all() and sel[raw[1] - w.id_base].all() and (~sel[ids - w.id_base]).any()
                for nq in (5, DIM_NQ):
                    kw = dict(workspace=ws, masks=None if sel is None else [w.mk(sel)] * nq, include_self=include_self)
                    _eq(w.index.search_by_rows(ids[:nq], k, reweighted=False, **kw), raw, nq, (dim, k, nq, include_self, "raw"))
                    _eq(w.index.search_by_rows(ids[:nq], k, reweighted=True, **kw), rew, nq, (dim, k, nq, include_self, "reweighted"))
    finally:
        ws.close()


# ---- 10. the same bytes twice -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", DIMS)
def test_same_bytes_twice(worlds, dim):
    """one call of every entry point, repeated: the same bytes in every output array"""
    w = worlds(dim)
    group_of = _groupings(w.n)["hashed"]
    grouping, fusion, boost = w.index.grouping(group_of.astype(np.int32)), w.index.fusion(256), w.index.boost_workspace(128)
    wide, rec = _native.IcdWide(w.index, DIM_NQ, 512), _native.IcdRecommend(w.index, 16, None, 512)
    rank, byr = _native.IcdRankOf(w.index), w.index.byrows(128)
    half = w.mk(((w.rows * 2654435761) >> 7) & 1 == 1)
    off = np.concatenate([[0], np.cumsum(LIST_SIZES)]).astype(np.int64)
    qv = np.ascontiguousarray(w.q[np.array(LIST_VECTORS)])
    hq = np.ascontiguousarray(w.q[_hybrid_sel(65)])
    table = w.mk.boosts([[(w.rows % 3 == 0, F(1.5)), (w.rows % 7 == 3, F(0.5))]] * DIM_NQ)
    reqs = _requests(w)
    ids = w.id_base + np.concatenate([500 + np.arange(20), np.arange(0, 500, 10)]).astype(np.int64)
    calls = {
        "grouped": lambda: w.index.search_grouped(w.q, 10, 2, grouping),
        "sum scorer": lambda: w.index.search_grouped(w.q, 10, 3, grouping, scorer="sum", group_scores=True),
        "MAX_SIM": lambda: w.index.search_lists(qv, off, 10, grouping, scorer="mean"),
        "hybrid": lambda: w.index.search_hybrid(hq, [128, 128], 128, fusion, ranker="weighted", weights=ATAN_W, norm="atan", masks=[[half, None]] * 65),
        "hybrid grouped": lambda: w.index.search_hybrid(hq, [5, 3], 5, fusion, grouping=grouping, group_size=3),
        "boosted": lambda: w.index.search_boosted(w.q, 17, table, [half] * DIM_NQ, workspace=boost),
        "wide": lambda: wide.search_wide(w.q, 400, first=100, masks=[half] * DIM_NQ),
        "recommend": lambda: rec.recommend([r[0] for r in reqs], [r[1] for r in reqs], "average_vector", 300),
        "rank-of": lambda: rank.rank_of(w.q, _targets(w, DIM_NQ, 16), [half] * DIM_NQ),
        "by-rows": lambda: w.index.search_by_rows(ids, 127, workspace=byr, masks=[half] * len(ids)),
    }
    try:
        for name, call in calls.items():
            first = [(_np(a).dtype, _np(a).shape, _bits(a)) for a in call()]
            for _ in range(2):
                assert [(_np(a).dtype, _np(a).shape, _bits(a)) for a in call()] == first, (dim, name)
    finally:
        for h in (grouping, fusion, boost, wide, rec, rank, byr):
            h.close()
