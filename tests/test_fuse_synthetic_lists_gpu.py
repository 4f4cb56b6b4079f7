"""hybrid_fuse_kernel and hybrid_fuse_grouped_kernel (csrc/hybrid_fuse.hpp) on lists no search of the index produces (run with -m gpu on
an MI355X): IcdIndex.fuse_lists over tests/fuse_list_cases.py's synthetic lists against hybrid_oracle.fuse_query and
grouped_hybrid_oracle.fuse_query_grouped, byte for byte (ids, levels, request bits, groups, fused and adjusted doubles; atan alone
under test_hybrid_search_gpu's tolerance rule). Every width of the sort network from 2 to 1024; lists that are disjoint, identical,
rotated, full of repeats (one query: ONE id in all R * lmax slots), holed, empty and short of k; scores that are negative, cancel to
0.0, are signed zeros, subnormal, huge, +inf, tied and of magnitudes 1e-30 .. 1e30 in one run; batches of 1, 3 and 300 through the host staging; an id_base above 2^32 and a
view asked for ids between its own; groupings and group runs that alternate, outlast s and are split by holes.
A 300-row, dim-32 index: the kernels never read a vector. Every case's aim is asserted on the oracle's answer first
(fuse_list_cases.assert_*; tests/test_fuse_list_cases_cpu.py asserts all of them without a GPU). DESIGN.md sections 13 - 15."""
import numpy as np
import pytest

import fuse_list_cases as fc
import grouped_hybrid_oracle as gho
from conftest import icd_levels, unit_rows
from hybrid_oracle import fuse_query

pytestmark = pytest.mark.gpu

from rag_project_icd10_amd._native import IcdIndex  # noqa: E402

N, DIM, MAX_TOTAL = 300, 32, 8 * 300
ID_BASE = 2 ** 32 + 12345
VIEW_ROWS = np.arange(1, N - 1, 3, dtype=np.int64)   # every third row; rows 0 and 299 lie outside: ids below its first and above its last
LEVELS = icd_levels(N, 11)
W_COSINE = [0.3, 1.0, 0.7, 0.9, 0.2, 0.6, 0.1, 0.8]
RANKERS = (("rrf", fc.W_ONES, "none"), ("weighted", fc.W_MIXED, "none"), ("weighted", W_COSINE, "cosine"))
_CACHE = {}


def _index(id_base):
    if id_base not in _CACHE:
        index = IcdIndex(unit_rows(N, DIM, 5), LEVELS, max_nq=MAX_TOTAL, max_k=128, id_base=id_base, probe=False)
        _CACHE[id_base] = (index, index.fusion(MAX_TOTAL))
    return _CACHE[id_base]


def _view():
    if "view" not in _CACHE:
        view = _index(ID_BASE)[0].view(VIEW_ROWS, max_nq=MAX_TOTAL, max_k=128)
        _CACHE["view"] = (view, view.fusion(MAX_TOTAL))
    return _CACHE["view"]


def _grouping(gname):
    if ("g", gname) not in _CACHE:
        _CACHE[("g", gname)] = _index(0)[0].grouping(fc.groupings(N)[gname], max_nq=MAX_TOTAL)
    return _CACHE[("g", gname)]


def _kw(ranker, weights, norm, R):
    return {"ranker": "rrf", "rrf_c": 60.0} if ranker == "rrf" else {"ranker": "weighted", "weights": weights[:R], "norm": norm}


def _okw(ranker, weights, norm, R):
    return {"ranker": "rrf", "c": 60.0} if ranker == "rrf" else {"ranker": "weighted", "weights": weights[:R], "norm": norm}


def _want(sc, ids, limits, k, okw, id_base):
    """the oracle per query -> (raw tuple, reweighted tuple) of [nq, k] arrays"""
    outs = [fuse_query(fc.cut(sc, ids, q, limits), LEVELS, k, id_base=id_base, n=N, **okw) for q in range(ids.shape[0])]
    return tuple(np.stack([o[0][j] for o in outs]) for j in range(4)), tuple(np.stack([o[1][j] for o in outs]) for j in range(5))


def _same(got, want, what):
    assert len(got) == len(want), what
    for j, (g, w) in enumerate(zip(got, want)):
        g = g.cpu().numpy() if hasattr(g, "cpu") else g
        if g.dtype == np.int32 and w.dtype == np.uint32:
            g = g.view(np.uint32)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, j, g.dtype, w.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (what, j, np.nonzero((g != w).any(1))[0][:5])


def _check(index, fusion, sc, ids, limits, k, kw, want, what, to_host=False, **grouped):
    _same(index.fuse_lists(fusion, sc, ids, limits, k, reweighted=False, to_host=to_host, **kw, **grouped), want[0], what + ("raw",))
    _same(index.fuse_lists(fusion, sc, ids, limits, k, reweighted=True, to_host=to_host, **kw, **grouped), want[1], what + ("reweighted",))


def _measures(sc, ids, limits, okw, id_base=0):
    R, lmax = ids.shape[1:]
    return [fc.measure(fuse_query(fc.cut(sc, ids, q, limits), LEVELS, R * lmax, id_base=id_base, n=N, **okw)[0], sc, ids, q, limits, N, id_base)
            for q in range(ids.shape[0])]


def _sweep(index, fusion, kinds, R, lmax, id_base, oracle_ids=lambda ids: ids, aims=True):
    for kind in kinds:
        sc, ids = fc.build(kind, 3, R, lmax, N, id_base, seed=R * 1000 + lmax)
        oids = oracle_ids(ids)
        for limits in fc.limit_sets(R, lmax):
            for ranker, weights, norm in RANKERS:
                okw = _okw(ranker, weights, norm, R)
                if aims and norm == "none":
                    ms = _measures(sc, oids, limits, okw, id_base)
                for k in (1, 10, 128):
                    if aims and norm == "none":
                        fc.assert_list_aim(kind, ms, R, lmax, limits, k, ranker)
                    want = _want(sc, oids, limits, k, okw, id_base)
                    _check(index, fusion, sc, ids, limits, k, _kw(ranker, weights, norm, R), want, (kind, R, lmax, tuple(limits), k, ranker, norm))


@pytest.mark.parametrize("R,lmax", fc.WIDTHS)
def test_every_sort_width(R, lmax):
    index, fusion = _index(0)
    _sweep(index, fusion, ("disjoint", "identical", "rotated", "holes", "few"), R, lmax, 0)


@pytest.mark.parametrize("score", [s for s in fc.SCORE_KINDS if s != "plain"])
@pytest.mark.parametrize("R,lmax", [(3, 43), (8, 128)])
def test_score_kinds(R, lmax, score):
    index, fusion = _index(0)
    limits = [lmax] * R
    for kind in ("rotated", "repeats"):
        sc, ids = fc.build(kind, 3, R, lmax, N, 0, seed=R + lmax, scores=score)
        for weights in (fc.W_MIXED, fc.W_ONES):
            for norm in ("none", "cosine"):
                okw = _okw("weighted", weights, norm, R)
                ms = _measures(sc, ids, limits, okw)
                fc.assert_list_aim(kind, ms, R, lmax, limits, 128, "weighted")
                fc.assert_score_aim(score, ms, R, weights, norm, kind)
                for k in (10, 128):
                    _check(index, fusion, sc, ids, limits, k, _kw("weighted", weights, norm, R), _want(sc, ids, limits, k, okw, 0), (score, kind, R, lmax, k, norm))


@pytest.mark.parametrize("score", ["negative", "huge"])
@pytest.mark.parametrize("R,lmax", [(3, 43), (8, 128)])
def test_weighted_atan_on_negative_and_huge_scores(R, lmax, score):
    """test_hybrid_search_gpu.test_weighted_atan_within_1e_12_of_the_oracle's rule, as it stands there: fused scores within 1e-12
    absolute (at most 8 terms with weights <= 1, each a few ulp of a value below 1 - so on `rotated`, whose runs hold at most R = 8
    terms), ids, levels and bits wherever the oracle's neighbouring fused scores differ by more than 1e-9. Values only: how many
    ranks are clear is not asserted (atan of a huge score is +-pi/2 to the last bit, and the fused scores then tie in blocks)."""
    index, fusion = _index(0)
    limits = [lmax] * R
    sc, ids = fc.build("rotated", 3, R, lmax, N, 0, seed=R + lmax, scores=score)
    for k in (10, 128):
        (wf, wi, wl, wb), _ = _want(sc, ids, limits, k, _okw("weighted", W_COSINE, "atan", R), 0)
        fused, got_ids, lv, bits = index.fuse_lists(fusion, sc, ids, limits, k, ranker="weighted", weights=W_COSINE[:R], norm="atan", reweighted=False, to_host=True)
        valid = wi >= 0
        assert np.array_equal(got_ids >= 0, valid) and valid.any()
        err = np.abs(fused[valid] - wf[valid]).max()
        print(f"atan {score} R={R} lmax={lmax} k={k}: max |fused - oracle| = {err:.3e}")
        assert err <= 1e-12
        with np.errstate(invalid="ignore"):   # (-inf - -inf in the padding)
            gap_prev = np.concatenate([np.full((3, 1), np.inf), np.abs(np.diff(wf, axis=1))], axis=1)
            gap_next = np.concatenate([np.abs(np.diff(wf, axis=1)), np.full((3, 1), np.inf)], axis=1)
        clear = valid & (np.nan_to_num(gap_prev, nan=np.inf) > 1e-9) & (np.nan_to_num(gap_next, nan=np.inf) > 1e-9)
        assert np.array_equal(got_ids[clear], wi[clear]) and np.array_equal(lv[clear], wl[clear]) and np.array_equal(bits[clear], wb[clear])


@pytest.mark.parametrize("nq", [1, 3, 300])
def test_batches_and_outputs(nq):
    """repeats + cancel at (8, 128), an empty query in the middle of the batch; 300 queries with host outputs pass the 256-query
    staging block twice; host outputs, device outputs and the same call a second time give the same bytes"""
    index, fusion = _index(0)
    R, lmax = 8, 128
    limits = [lmax] * R
    ids = fc.build_ids("repeats", nq, R, lmax, N, 0, seed=nq)
    if nq >= 3:
        e = fc.empty_query(nq)
        ids[e] = fc.build_ids("empty", 3, R, lmax, N, 0, seed=nq)[fc.empty_query(3)]
    sc = fc.build_scores("cancel", ids, nq)
    for weights, ks in ((fc.W_ONES, (10, 128)), (fc.W_MIXED, (128,))):
        okw = _okw("weighted", weights, "none", R)
        for k in ks:
            want = _want(sc, ids, limits, k, okw, 0)
            if nq >= 3:
                assert (want[0][1][e] == -1).all() and want[0][1][e - 1][0] >= 0 and want[0][1][e + 1][0] >= 0   # zero heads between heads
            assert want[0][1][0][0] >= 0 and want[0][1][0][1] == -1   # ONE head from 1024 slots
            kw = _kw("weighted", weights, "none", R)
            for _ in range(2):
                _check(index, fusion, sc, ids, limits, k, kw, want, ("batch", nq, k, "host"), to_host=True)
                _check(index, fusion, sc, ids, limits, k, kw, want, ("batch", nq, k, "device"))


WIDTHS_REDUCED = ((2, 1), (7, 9), (3, 43), (8, 128))


@pytest.mark.parametrize("R,lmax", WIDTHS_REDUCED)
def test_with_an_id_base_above_2_to_the_32(R, lmax):
    index, fusion = _index(ID_BASE)
    _sweep(index, fusion, ("holes", "repeats"), R, lmax, ID_BASE)


@pytest.mark.parametrize("R,lmax", WIDTHS_REDUCED)
def test_on_a_view_asked_for_ids_between_its_own(R, lmax):
    """the lists hold ids of the PARENT: those of the view's rows are hits, the others - between two of the view's ids, below its
    first, above its last - are skipped like padding and keep their slot (include/icd_search.h: "an id outside the index is skipped
    like padding"; hybrid_local_row's binary search through row_map). The oracle: fuse_query over the lists with every non-view id
    replaced by -1; levels through the parent."""
    view, vf = _view()
    keep = VIEW_ROWS + ID_BASE
    sc, ids = fc.build("repeats", 3, R, lmax, N, ID_BASE, seed=R * 1000 + lmax)
    rows = ids[(ids >= ID_BASE) & (ids < ID_BASE + N)] - ID_BASE
    if R * lmax >= 63:
        assert (rows % 3 != 1).any() and (rows % 3 == 1).any()           # parent ids between the view's, and the view's own
    sc, ids = fc.build("holes", 3, 8, 128, N, ID_BASE, seed=8128)         # (every row of the parent occurs: 0 and 299 too)
    rows = ids[(ids >= ID_BASE) & (ids < ID_BASE + N)] - ID_BASE
    assert 0 in rows and N - 1 in rows and VIEW_ROWS[0] == 1 and VIEW_ROWS[-1] == N - 2
    _sweep(view, vf, ("holes", "repeats"), R, lmax, ID_BASE, oracle_ids=lambda i: fc.restrict_to(i, keep), aims=False)
    # a list of every parent id in turn, one per slot: exactly the view's rows come back
    if (R, lmax) == (8, 128):
        allids = np.full((1, 8, 128), -1, np.int64)
        allids.reshape(-1)[:N] = np.arange(N) + ID_BASE
        ones = np.ones(allids.shape, np.float32)
        _f, got, _l, _b = view.fuse_lists(vf, ones, allids, [128] * 8, 128, ranker="weighted", weights=fc.W_ONES, norm="none", reweighted=False, to_host=True)
        assert np.array_equal(got[0][:len(keep)], keep) and (got[0][len(keep):] == -1).all()


def _want_grouped(sc, ids, group_of, limits, k, s, okw):
    outs = [gho.fuse_query_grouped([(sc[q, r], ids[q, r]) for r in range(ids.shape[1])], group_of, LEVELS, limits, k, s, **okw) for q in range(ids.shape[0])]
    return tuple(np.stack([o[0][j] for o in outs]) for j in range(5)), tuple(np.stack([o[1][j] for o in outs]) for j in range(6))


@pytest.mark.parametrize("R,lmax", fc.GROUPED_WIDTHS)
@pytest.mark.parametrize("gname", ["own", "one", "mod7", "fam20"])
def test_grouped_fuse(gname, R, lmax):
    index, fusion = _index(0)
    group_of = fc.groupings(N)[gname]
    g = _grouping(gname)
    few_groups = few_members = negative = False
    settings = [(r, w, nm, "plain") for r, w, nm in RANKERS] + [("weighted", fc.W_ONES, "none", "cancel"), ("weighted", fc.W_MIXED, "none", "negative")]
    for k, s in fc.KS:
        limits = fc.grouped_limits(R, lmax, s)
        for kind in fc.GROUPED_KINDS:
            ids = fc.build_grouped_ids(kind, 3, R, lmax, group_of, s, limits, seed=R + lmax + k)
            for ranker, weights, norm, score in settings:
                sc = fc.build_scores(score, ids, 3)
                want = _want_grouped(sc, ids, group_of, limits, k, s, _okw(ranker, weights, norm, R))
                for q in range(3):
                    ng, least = fc.groups_and_members([w[q] for w in want[0]], k, s)
                    few_groups |= 0 < ng < k
                    few_members |= 0 < least < s
                if kind == "empty":
                    assert (want[0][1][1] == -1).all() and want[0][1][0][0] >= 0
                if score == "negative":
                    assert (want[0][0][np.isfinite(want[0][0])] <= 0).all()
                    negative |= bool((want[0][0][np.isfinite(want[0][0])] < 0).any())
                _check(index, fusion, sc, ids, limits, k, _kw(ranker, weights, norm, R), want, (gname, kind, R, lmax, k, s, ranker, norm, score),
                       grouping=g, group_size=s)
    assert negative
    if (R, lmax) == (8, 128):    # the aim: fewer groups than k, and a group of fewer than s members, both in the oracle's answers
        assert few_groups or gname == "own"
        assert few_members or gname == "one"


@pytest.mark.parametrize("kind", ["abab", "repeats"])
def test_grouped_fuse_of_300_queries(kind):
    index, fusion = _index(0)
    group_of = fc.groupings(N)["mod7"]
    g = _grouping("mod7")
    R, lmax, k, s, nq = 8, 128, 10, 3, 300
    limits = fc.grouped_limits(R, lmax, s)
    ids = fc.build_grouped_ids(kind, nq, R, lmax, group_of, s, limits, seed=300)
    if kind == "repeats":
        ids[fc.empty_query(nq)] = -1
    sc = fc.build_scores("cancel" if kind == "repeats" else "plain", ids, 300)
    ranker, weights, norm = ("weighted", fc.W_ONES, "none") if kind == "repeats" else RANKERS[0]
    want = _want_grouped(sc, ids, group_of, limits, k, s, _okw(ranker, weights, norm, R))
    _check(index, fusion, sc, ids, limits, k, _kw(ranker, weights, norm, R), want, (kind, 300, "host"), to_host=True, grouping=g, group_size=s)
    _check(index, fusion, sc, ids, limits, k, _kw(ranker, weights, norm, R), want, (kind, 300, "device"), grouping=g, group_size=s)
