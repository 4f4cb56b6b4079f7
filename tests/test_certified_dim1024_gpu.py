"""The certified search (fp16 coarse sweep -> certifying finalize -> exact re-search of what it cannot clear) at dim 1024 on every
route tests/test_gpu_parity.py takes at dim 768 only.

The two fast-path dims do not run the same kernels: at 1024 the first pass is coarse_flat_kernel<1024, CF_PRODUCT_VAR & (3 | 16 |
2048)> - the 32x32x16 MFMA form, no pinned query fragments, no two-step fragment prefetch, 32 stages per tile, 64 query
fragments per lane -, the second pass its own persistent instantiation, every k from 33 to 100 runs on lists of 16 (the wide
lists are a dim-768 rule), and finalize's per-wave LDS block and the certificate's dim terms are larger.

Every case is parametrised over dim in (768, 1024): 768 is the control that shows the SHAPE reaches the route it is named after,
1024 is the coverage. Each case asserts that route from index.stats() at both dims, and where the precondition is a property of
the list plan (tests/flat_partition_check.cpp `plan`, built with g++) it is asserted from the planner too:
test_list_plan_preconditions runs those without a GPU.

Bar: the project's own. Ids exact, raw scores bit-identical fp32, reweighted scores bit-identical float64, levels equal; no
tolerance anywhere. Shapes: the smallest at which the route is still reached (a few seconds per case).
"""
import functools

import numpy as np
import pytest

from conftest import icd_levels, unit_rows
from test_flat_partition import build_checker, coarse_plan
from test_gpu_parity import _check, _family_corpus, _tight_family_corpus

from rag_project_icd10_amd._native import MODE_AUTO, MODE_EXACT, IcdIndex  # noqa: E402

gpu = pytest.mark.gpu
DIMS = (768, 1024)
dims = pytest.mark.parametrize("dim", DIMS)

# rag_project_icd10_amd/csrc: flat_partition.hpp, coarse_common.hpp, coarse_flat_kernel.hpp, finalize.hpp
CO_KP, CO_KP_WIDE, FIN_MAX_CAND = 16, 24, 512
PASS2_BELOW = 320          # the second pass is planned when the first gives a query fewer candidates than this
WIDE_RETRY_FROM = 128      # the wide-window retry runs when a query's lists hold at least this many candidates (k <= 32)
EPOCH = 24                 # tiles between two synchronised compactions of all queries of a work-group (VAR bit 2048)


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


@functools.lru_cache(maxsize=None)
def _rows(n, dim, seed):
    """unit_rows, generated once per (shape, seed) and shared read-only"""
    x = unit_rows(n, dim, seed)
    x.setflags(write=False)
    return x


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    return build_checker(tmp_path_factory.mktemp("flat_partition"))


def _kp(dim, k):
    """candidates per list of the first pass: 24 above k = 48 at dim 768 only (icd_search.hip auto_plan, opt_wide_from)"""
    return CO_KP_WIDE if (k > 48 and dim == 768) else CO_KP


# ---- the list plans the cases rely on (no GPU) ----------------------------------------------------------------------------
K_NARROW = (13, 20, 32, 33, 48, 64, 100)
PASS2_NQ = 2049            # case 7: 17 query tiles x 16 corpus tiles = 272 units > 256 CUs -> two tiles per work-group, 8 lists


def _plan_every_k(planner, dim, k):
    p = coarse_plan(planner, 8192, dim, 150, k)
    assert p["ok"] == 1 and p["in_reach"] == 1, p
    assert 2 <= p["P"] <= 32 and p["P"] * _kp(dim, k) <= FIN_MAX_CAND, p
    return p


def _plan_compaction(planner, dim):
    """icd_index_set_chunks(2) (plan_coarse_lists, chunks_override): ceil(ctiles / 2) tiles per work-group, every work-group's
    run ONE list - the planner's `plan` command has no chunks argument, so the list length follows from its ctiles"""
    p = coarse_plan(planner, 8192, dim, 300, 10)
    assert p["ok"] == 1 and (p["ctiles"] + 1) // 2 >= EPOCH, p
    return p


def _plan_second_pass(planner, dim):
    p = coarse_plan(planner, 2000, dim, PASS2_NQ, 10)
    assert p["ok"] == 1 and p["P"] * CO_KP < PASS2_BELOW and p["P2"] > 0 and p["P2"] * CO_KP > p["P"] * CO_KP, p
    assert p["P"] * CO_KP >= WIDE_RETRY_FROM, p                         # (the retry runs first: the second pass reads flag word 1)
    assert coarse_plan(planner, 2000, dim, PASS2_NQ - 1, 10)["P2"] == 0   # one query tile less: 16 lists, no second pass planned
    wide = coarse_plan(planner, 2000, dim, PASS2_NQ, 10, wide_now=1)      # wide mode: the second pass's list count at once
    assert wide["ok"] == 1 and wide["P"] == p["P2"] and wide["P2"] == 0, wide
    return p


def _plan_families(planner, dim, n, nq, k):
    """batches below 2 048 queries: the lists fill the wide window (the retry runs) and no second pass is planned"""
    p = coarse_plan(planner, n, dim, nq, k)
    assert p["ok"] == 1 and p["P"] * CO_KP >= max(WIDE_RETRY_FROM, PASS2_BELOW) and p["P2"] == 0, p
    return p


@dims
def test_list_plan_preconditions(planner, dim):
    """the plan-derived preconditions of the cases below, at both dims, without a GPU"""
    for n in (129, 2049, 4097):
        for nq in (17, 128, 129, 300):
            for k in (1, 10, 16, 17, 32):
                p = coarse_plan(planner, n, dim, nq, k)
                assert p["ok"] == 1 and p["in_reach"] == 1 and p["ctiles"] >= (n + 127) // 128, (n, nq, k, p)
    for k in K_NARROW:
        _plan_every_k(planner, dim, k)
    if dim == 1024:   # what no 768 test covers: k > 48 on lists of 16, up to the 32 lists finalize's window holds
        assert _plan_every_k(planner, dim, 100)["P"] * CO_KP == FIN_MAX_CAND
    _plan_compaction(planner, dim)
    _plan_second_pass(planner, dim)
    for nq in (600, 130, 40):
        for k in (10, 20):
            _plan_families(planner, dim, 60 * 124, nq, k)


# ---- 1. ragged edges of both tilings ----------------------------------------------------------------------------------------
@gpu
@dims
@pytest.mark.parametrize("n", [129, 2049, 4097])
def test_ragged_corpus_and_query_tiles(oracle, n, dim):
    """a last corpus tile of ONE row (4 097: more tiles than the seven spare ones pad), and 17 queries (the first batch AUTO
    sweeps), a full query tile, one query in a second tile, a third tile; k = 1, at and across the 16-wide list, 32"""
    corpus, levels, queries = _rows(n, dim, 1000 + n), icd_levels(n, 1001 + n), _rows(300, dim, 1002 + n)
    idx = IcdIndex(corpus, levels, max_nq=300, max_k=32)
    for nq in (17, 128, 129, 300):
        for k in (1, 10, 16, 17, 32):
            st = _check(oracle, idx, corpus, levels, queries[:nq], k, MODE_AUTO)
            assert st["last_mode"] == MODE_AUTO and st["fast_path"] == 1 and st["dim"] == dim, (nq, k, st)
    idx.close()


# ---- 2. every k on narrow lists --------------------------------------------------------------------------------------------
@gpu
@dims
@pytest.mark.parametrize("k", K_NARROW + (101,))
def test_every_k_on_narrow_lists(oracle, planner, k, dim):
    """8 192 Gaussian rows, 150 queries (a second query tile). At dim 1024 k > 48 runs on 16-wide lists - up to 32 of them,
    finalize's whole candidate window at k = 100 - where dim 768 takes 24-wide ones. Fewer than half of the queries may take the
    exact re-search: a batch that fell back as a whole is not a certified one. k = 101 is past the fast path."""
    n, nq = 8192, 150
    corpus, levels, queries = _rows(n, dim, 1100), icd_levels(n, 1101), _rows(nq, dim, 1102)
    idx = IcdIndex(corpus, levels, max_nq=nq, max_k=128)
    st = _check(oracle, idx, corpus, levels, queries, k, MODE_AUTO)
    if k > 100:
        assert st["last_mode"] == MODE_EXACT
    else:
        plan = _plan_every_k(planner, dim, k)
        print(f"every k: dim {dim} k {k}: {st['last_chunks']} lists of {_kp(dim, k)}, exact re-search for {st['last_fallback']} of {nq}")
        assert st["last_mode"] == MODE_AUTO and st["last_chunks"] == plan["P"], (st, plan)
        assert st["last_fallback"] < nq // 2, st
    idx.close()


# ---- 3. the synchronised compaction ----------------------------------------------------------------------------------------
@gpu
@dims
@pytest.mark.parametrize("dups", [False, True])
def test_synchronised_compaction_at_tile_24(oracle, planner, dups, dim):
    """8 192 rows under icd_index_set_chunks(2): two lists of 32 tiles per query, so the all-queries compaction at tile 24 runs,
    on unique scores and with a fifth of the rows duplicated (ties at a buffer's KP-th place); 300 queries = three query tiles"""
    n, nq = 8192, 300
    corpus = _rows(n, dim, 1200)
    if dups:
        corpus = corpus.copy()
        corpus[5::5] = corpus[np.arange(5, n, 5) // 2]
    levels, queries = icd_levels(n, 1201), _rows(nq, dim, 1202)
    ctiles = _plan_compaction(planner, dim)["ctiles"]
    idx = IcdIndex(corpus, levels, max_nq=nq, max_k=10)
    idx.set_chunks(2)
    st = _check(oracle, idx, corpus, levels, queries, 10, MODE_AUTO)
    assert st["last_mode"] == MODE_AUTO and st["last_chunks"] >= 2, st
    assert -(-ctiles // st["last_chunks"]) >= EPOCH, (ctiles, st)          # the longest of a query's lists, at least
    if not dups:
        assert st["last_fallback"] == 0
    idx.close()


# ---- 4. the select's tie path ----------------------------------------------------------------------------------------------
@gpu
@dims
def test_the_selects_tie_path(oracle, dim):
    """40 identical rows that are every query's best hits: all their coarse scores tie, the ballot bisection cannot split them
    and the select ranks by unique keys; ids come out row-ascending"""
    corpus = _rows(5000, dim, 1300).copy()
    corpus[100:140] = corpus[100]
    rng = np.random.default_rng(1301)
    queries = corpus[100][None, :] + 0.03 * rng.standard_normal((150, dim)).astype(np.float32)
    queries = np.ascontiguousarray(queries / np.linalg.norm(queries, axis=1, keepdims=True), dtype=np.float32)
    levels = icd_levels(5000, 1302)
    idx = IcdIndex(corpus, levels, max_nq=150, max_k=10)
    st = _check(oracle, idx, corpus, levels, queries, 10, MODE_AUTO)
    assert st["last_mode"] == MODE_AUTO
    s, i = idx.search(queries, 10, MODE_AUTO)
    assert np.array_equal(i, np.tile(np.arange(100, 110), (150, 1)))
    idx.close()


# ---- 5. exact ties broken by id, with an id_base --------------------------------------------------------------------------
@gpu
@dims
@pytest.mark.parametrize("id_base", [1_000_000, 2 ** 32 + 12_345])
def test_exact_ties_with_an_id_base(oracle, id_base, dim):
    """duplicate rows: exact score ties, broken by id; the ids carry a base, one of them past 32 bits"""
    n = 3001
    corpus = _rows(n, dim, 1400).copy()
    corpus[5::5] = corpus[np.arange(5, n, 5) // 2]
    levels, queries = icd_levels(n, 1401), _rows(70, dim, 1402)
    idx = IcdIndex(corpus, levels, max_nq=70, max_k=10, id_base=id_base)
    for mode in (MODE_AUTO, MODE_EXACT):
        st = _check(oracle, idx, corpus, levels, queries, 10, mode, id_base=id_base)
        assert st["last_mode"] == mode and st["id_base"] == id_base, st
    idx.close()


# ---- 6. both fallback routes -----------------------------------------------------------------------------------------------
@gpu
@dims
def test_both_fallback_routes(oracle, dim):
    """300 all-zero queries of 900 (every score ties at 0, nothing certifies): a dense flagged list, the fp32-MFMA exact kernel
    at this dim; 100 of 300: the streaming kernel in passes of 8"""
    corpus, levels = _rows(3000, dim, 1500), icd_levels(3000, 1501)
    queries = _rows(900, dim, 1502).copy()
    queries[::3] = 0.0
    idx = IcdIndex(corpus, levels, max_nq=900, max_k=10)
    st = _check(oracle, idx, corpus, levels, queries, 10, MODE_AUTO)
    assert st["last_mode"] == MODE_AUTO and st["last_fallback"] == 300, st
    st = _check(oracle, idx, corpus, levels, queries[:300], 10, MODE_AUTO)
    assert st["last_mode"] == MODE_AUTO and st["last_fallback"] == 100, st
    idx.close()


# ---- 7. the persistent second pass -----------------------------------------------------------------------------------------
@gpu
@dims
def test_persistent_second_pass(oracle, planner, dim):
    """10 distinct rows x 200 copies, no create probe: every candidate list overflows with exact ties and the first pass (with
    its wide-window retry) certifies nobody. 2 049 queries is the smallest batch the planner gives a second pass (one query
    tile less has 16 lists of its own: _plan_second_pass): 8 lists in the first pass, 16 in the second, whose persistent
    kernel sweeps for all 2 049 - the last query tile holds ONE query. Same bytes with the second pass, without it (everything
    to the dense exact re-search) and from MODE_EXACT; the batch after it is planned in wide mode."""
    nq = PASS2_NQ
    plan = _plan_second_pass(planner, dim)
    corpus, levels = np.repeat(_rows(10, dim, 1600), 200, axis=0), icd_levels(2000, 1601)
    queries = _rows(nq, dim, 1602)
    idx = IcdIndex(corpus, levels, max_nq=nq, max_k=10, probe=False)
    idx.set_second_pass(False)
    s0, i0 = idx.search(queries, 10, MODE_AUTO)
    st0 = idx.stats()
    assert st0["last_mode"] == MODE_AUTO and st0["last_chunks"] == plan["P"], (st0, plan)
    assert st0["last_second_pass_lists"] == 0 and st0["last_fallback"] == nq, st0
    se, ie = idx.search(queries, 10, MODE_EXACT)
    assert idx.stats()["last_mode"] == MODE_EXACT
    idx.set_second_pass(True)
    s2, i2 = idx.search(queries, 10, MODE_AUTO)
    st2 = idx.stats()
    print(f"second pass: dim {dim}: {st2['last_second_pass']} of {nq} queries into the second pass ({st2['last_second_pass_lists']} lists), "
          f"exact re-search for {st2['last_fallback']}; {st0['last_fallback']} without it")
    assert st2["last_mode"] == MODE_AUTO and st2["wide_mode"] == 0 and st2["last_chunks"] == plan["P"], (st2, plan)
    assert st2["last_second_pass_lists"] == plan["P2"] and st2["last_second_pass"] == nq and st2["last_fallback"] < nq, st2
    assert np.array_equal(i2, i0) and _bits(s2) == _bits(s0)
    assert np.array_equal(ie, i0) and _bits(se) == _bits(s0)
    sample = np.arange(0, nq, 37)
    os_, oi = oracle.flat_ip_topk(corpus, queries[sample], 10)
    assert np.array_equal(i2[sample], oi) and _bits(s2[sample]) == _bits(os_)
    # the next large batch: the counters of that one have arrived (stats waited for them), it is planned wide from the start -
    # the second pass's list count in the first pass, every query through the widest window at once
    adj, raw, ids, lv = idx.search_reweighted(queries, 10, MODE_AUTO)
    st3 = idx.stats()
    assert st3["wide_mode"] == 1 and st3["last_chunks"] == plan["P2"] and st3["last_second_pass_lists"] == 0, st3
    want = oracle.reweight(os_, oi, levels)
    assert np.array_equal(ids[sample], want[2]) and _bits(adj[sample]) == _bits(want[0]) and _bits(raw[sample]) == _bits(want[1])
    assert np.array_equal(lv[sample], want[3])
    idx.close()


# ---- 8. families and the wide window ---------------------------------------------------------------------------------------
FAMILY_BATCHES = (600, 130, 40)
_family_fallbacks = {}     # (dim, k) -> {batch: last_fallback}: the dim-768 run is the yardstick of the dim-1024 one


def _family_run(oracle, planner, dim, k):
    """60 families of 124 rows of mutual cosine ~0.99, in code order: a query has its whole family within 2 eps of its k-th
    best, more candidates than the window sized for k holds, so the first finalize flags it and the wide-window retry (256
    candidates from the same lists) certifies it. Checked against the oracle; returns the exact re-searches per batch."""
    if (dim, k) in _family_fallbacks:
        return _family_fallbacks[(dim, k)]
    corpus, queries = _tight_family_corpus(60, 124, dim, 0.10, 600, 1700)
    levels = icd_levels(len(corpus), 1701)
    idx = IcdIndex(corpus, levels, max_nq=600, max_k=k)
    out = {}
    for nq in FAMILY_BATCHES:
        plan = _plan_families(planner, dim, len(corpus), nq, k)
        st = _check(oracle, idx, corpus, levels, queries[:nq], k, MODE_AUTO)
        assert st["last_mode"] == MODE_AUTO and st["last_second_pass_lists"] == 0, st
        assert st["last_chunks"] == plan["P"], (st, plan)
        out[nq] = int(st["last_fallback"])
    idx.close()
    _family_fallbacks[(dim, k)] = out
    return out


@gpu
@dims
@pytest.mark.parametrize("k", [10, 20])
def test_tight_families_through_the_wide_window(oracle, planner, k, dim):
    """Bytes equal to the oracle at 600, 130 and 40 queries (_family_run). No count of exact re-searches can be derived for
    this corpus, so the dim-768 run of the same case in the same session is the yardstick: dim 1024 may send at most twice as
    many queries to the exact re-search, or that many plus 1 % of the batch, whichever is larger."""
    got = _family_run(oracle, planner, dim, k)
    ref = _family_run(oracle, planner, 768, k)
    print(f"tight families k={k}: exact re-searches per batch {FAMILY_BATCHES}: dim {dim} {[got[b] for b in FAMILY_BATCHES]}, "
          f"dim 768 {[ref[b] for b in FAMILY_BATCHES]}")
    for nq in FAMILY_BATCHES:
        assert got[nq] <= max(2 * ref[nq], ref[nq] + nq // 100), (nq, got, ref)


@gpu
@dims
def test_families_in_code_order_with_and_without_the_row_permutation(oracle, dim):
    """60 looser families of 120 NEIGHBOURING rows: the fp16 image is stored in a permuted row order so that a family spreads
    over the candidate lists; in row order one list holds the family and ends on a bound inside it. Exact either way, and the
    row-order image never certifies more."""
    corpus, queries = _family_corpus(60, 120, dim, 1750)
    levels = icd_levels(len(corpus), 1751)
    fall = {}
    for permute in (True, False):
        idx = IcdIndex(corpus, levels, max_nq=256, max_k=10, permute=permute)
        st = _check(oracle, idx, corpus, levels, queries, 10, MODE_AUTO)
        assert st["last_mode"] == MODE_AUTO, st
        fall[permute] = int(st["last_fallback"])
        idx.close()
    print(f"families in code order: dim {dim}: exact re-search for {fall[True]} of 256 queries permuted, {fall[False]} in row order")
    assert fall[False] >= fall[True]


# ---- 9. the centred image --------------------------------------------------------------------------------------------------
@gpu
@dims
@pytest.mark.parametrize("k", [10, 20])
def test_anisotropic_rows_on_a_centred_image(oracle, k, dim):
    """unit rows = a common direction + noise of norm ~0.2 (cosine of two rows ~0.96): icd_index_create centres the fp16 image
    (q.c = q.(c - mu) + q.mu) and the certificate's window is relative to the centred norms. 8 192 rows, 300 queries: the
    centred image certifies the batch (at most 5 % re-searched, never more than uncentred). At this corpus size the uncentred
    image still certifies most queries too (measured: 0 / 0 of 300 re-searched at k = 10 at dim 768 / 1024, 1 / 42 at k = 20),
    so the case checks the centred image's arithmetic - that centring was taken is asserted from the stats - not its benefit."""
    rng = np.random.default_rng(1800 + dim)
    n, nq = 8192, 300
    mu0 = rng.standard_normal(dim).astype(np.float32)
    mu0 /= np.linalg.norm(mu0)

    def rows(m):
        x = mu0[None, :] + (0.2 / np.sqrt(dim)) * rng.standard_normal((m, dim)).astype(np.float32)
        x /= np.linalg.norm(x, axis=1, keepdims=True)
        return np.ascontiguousarray(x, dtype=np.float32)

    corpus, queries = rows(n), rows(nq)
    levels = icd_levels(n, 1801)
    fall = {}
    for center in (1, 0):
        idx = IcdIndex(corpus, levels, max_nq=nq, max_k=k, center=bool(center))
        st = idx.stats()
        assert st["centered"] == center and st["mean_share"] > 0.5 and abs(st["rmax"] - 1.0) < 1e-3, st
        st = _check(oracle, idx, corpus, levels, queries, k, MODE_AUTO)
        assert st["last_mode"] == MODE_AUTO and st["fast_path"] == 1, st
        fall[center] = int(st["last_fallback"])
        idx.close()
    print(f"anisotropic rows: dim {dim} k {k}: exact re-search for {fall[1]} of {nq} queries centred, {fall[0]} uncentred")
    assert fall[1] <= nq // 20 and fall[1] <= fall[0]


# ---- 10. scaled norms ------------------------------------------------------------------------------------------------------
@gpu
@dims
@pytest.mark.parametrize("cscale,qscale", [(1e-5, 1.0), (1e-30, 1e-6), (1e12, 1e10), (3e-38, 1.0)])
def test_power_of_two_scaling_at_tiny_and_huge_norms(oracle, cscale, qscale, dim):
    """data far below fp16's normal range or above its largest value: the images are power-of-two scaled, the certificate's
    relative bound holds and the batch stays certified; near fp32's own underflow the bound's absolute term takes over and the
    exact kernels answer"""
    n, nq = 8192, 300
    corpus, levels = _rows(n, dim, 1900) * np.float32(cscale), icd_levels(n, 1901)
    queries = _rows(nq, dim, 1902) * np.float32(qscale)
    idx = IcdIndex(corpus, levels, max_nq=nq, max_k=10)
    assert idx.stats()["fast_path"] == 1
    st = _check(oracle, idx, corpus, levels, queries, 10, MODE_AUTO)
    assert st["last_mode"] == MODE_AUTO, st
    print(f"scaled norms: dim {dim} corpus x {cscale:g} queries x {qscale:g}: exact re-search for {st['last_fallback']} of {nq}")
    if cscale * qscale > 1e-30:
        assert st["last_fallback"] <= nq // 10, st        # certified on the fast path, not rescued by the exact re-search
    _check(oracle, idx, corpus, levels, queries[:5], 10, MODE_AUTO)
    idx.close()


@gpu
@dims
def test_mixed_magnitudes_within_one_corpus_and_batch(oracle, dim):
    """only SOME rows, components and queries are tiny: the corpus scale comes from its largest component, the tiny rows' fp16
    images sink into the subnormal range and the bound's absolute term covers them"""
    n, nq = 8192, 300
    rng = np.random.default_rng(1950)
    corpus, levels = _rows(n, dim, 1951).copy(), icd_levels(n, 1952)
    corpus[::3] *= np.float32(1e-6)
    corpus[1::7] *= np.float32(1e-3)
    corpus[:, :dim // 8] *= np.float32(1e-5)
    queries = _rows(nq, dim, 1953) * (10.0 ** rng.uniform(-6, 2, (nq, 1))).astype(np.float32)
    queries[::5] *= -1.0
    idx = IcdIndex(corpus, levels, max_nq=nq, max_k=10)
    st = _check(oracle, idx, corpus, levels, queries, 10, MODE_AUTO)
    assert st["last_mode"] == MODE_AUTO and st["fast_path"] == 1, st
    st = _check(oracle, idx, corpus, levels, queries, 5, MODE_EXACT)
    assert st["last_mode"] == MODE_EXACT
    idx.close()


# ---- 11. EXACT above k = 32 ------------------------------------------------------------------------------------------------
@gpu
@dims
@pytest.mark.parametrize("k", [33, 64, 100])
def test_exact_mode_above_k32_on_certified_narrow_lists(oracle, k, dim):
    """MODE_EXACT at k > 32: lists of 32 over row-strided chunks, finalize's narrow_check, re-search of what it cannot clear.
    8 192 rows are the 64 row tiles the route asks for, 200 queries more than the streaming kernel takes. Gaussian rows,
    families of NEIGHBOURING near-identical rows and 700 exact duplicates of one row certify without a re-search and equal the
    KP >= k lists (exact_narrow = 0); 45 copies of one query at rows 3, 3 + P, 3 + 2 P, ... put more than 32 members of its
    top-k into ONE strided chunk, which only this route's certificate can see: it must flag (last_fallback >= 1)."""
    n, nq = 8192, 200
    rng = np.random.default_rng(2000 + k)
    gauss = _rows(n, dim, 2100 + k)
    nfam = n // 120
    fam = np.repeat(rng.standard_normal((nfam, dim)).astype(np.float32), 120, axis=0)
    fam = fam + 0.1 * rng.standard_normal(fam.shape).astype(np.float32)
    fam = np.ascontiguousarray(fam / np.linalg.norm(fam, axis=1, keepdims=True), dtype=np.float32)
    dup = gauss.copy()
    dup[rng.choice(n, 700, replace=False)] = gauss[17]
    queries = _rows(nq, dim, 2200 + k).copy()
    queries[:40] = fam[np.arange(40) * 120 + 5] + 0.05 * rng.standard_normal((40, dim)).astype(np.float32)
    queries[40] = gauss[17]
    queries /= np.linalg.norm(queries, axis=1, keepdims=True)
    pn = None
    for name, corpus in (("gauss", gauss), ("families", fam), ("duplicates", dup)):
        levels = icd_levels(len(corpus), 2001)
        assert (len(corpus) + 127) // 128 >= 64
        idx = IcdIndex(corpus, levels, max_nq=nq, max_k=100)
        os_, oi = oracle.flat_ip_topk(corpus, queries, k)
        want = oracle.reweight(os_, oi, levels)
        for narrow in (1, 0):
            idx.set_option("exact_narrow", narrow)
            s, i = idx.search(queries, k, MODE_EXACT)
            got = idx.search_reweighted(queries, k, MODE_EXACT)
            assert np.array_equal(i, oi) and _bits(s) == _bits(os_), (name, narrow)
            assert np.array_equal(got[2], want[2]) and _bits(got[0]) == _bits(want[0]) and _bits(got[1]) == _bits(want[1]), (name, narrow)
            assert np.array_equal(got[3], want[3]), (name, narrow)
            if narrow:
                st = idx.stats()
                pn = st["last_chunks"]
                assert st["last_mode"] == MODE_EXACT and st["last_fallback"] == 0, (name, st)
        idx.close()
    adv = gauss.copy()
    adv[3 + pn * np.arange(45)] = queries[7]
    levels = icd_levels(n, 2001)
    idx = IcdIndex(adv, levels, max_nq=nq, max_k=100)
    os_, oi = oracle.flat_ip_topk(adv, queries, k)
    s, i = idx.search(queries, k, MODE_EXACT)
    st = idx.stats()
    assert st["last_mode"] == MODE_EXACT and st["last_chunks"] == pn and st["last_fallback"] >= 1, st
    assert np.array_equal(i, oi) and _bits(s) == _bits(os_)
    idx.close()


# ---- 12. one handle, many call shapes --------------------------------------------------------------------------------------
@gpu
@dims
def test_one_handle_many_call_shapes(oracle, dim):
    """the same handle serves batches of very different sizes, k and modes back to back, some with a 2e5 component in every
    seventh query (beyond fp16's range: the query's own scale absorbs it): workspaces, shared thresholds and device-side
    counters carry nothing over from call to call"""
    n = 8192
    corpus, levels = _rows(n, dim, 2300), icd_levels(n, 2301)
    queries = _rows(1000, dim, 2302)
    bad = queries.copy()
    bad[::7, 5] = 2e5
    idx = IcdIndex(corpus, levels, max_nq=1000, max_k=64)
    plan = [(1000, 10, MODE_AUTO, queries), (1, 10, MODE_AUTO, queries), (300, 5, MODE_AUTO, bad), (1000, 10, MODE_AUTO, bad),
            (17, 12, MODE_AUTO, queries), (700, 10, MODE_EXACT, queries), (129, 64, MODE_AUTO, queries), (1000, 10, MODE_AUTO, queries),
            (64, 1, MODE_EXACT, bad), (400, 10, MODE_AUTO, queries)]
    for nq, k, mode, src in plan:
        q = src[:nq]
        s, i = idx.search(q, k, mode)
        st = idx.stats()
        assert st["last_mode"] == (MODE_AUTO if mode == MODE_AUTO and nq > 16 else MODE_EXACT) and st["last_nq"] == nq, (nq, k, mode, st)
        sample = np.unique(np.concatenate([np.arange(0, nq, max(1, nq // 40)), [nq - 1]]))
        os_, oi = oracle.flat_ip_topk(corpus, q[sample], k)
        assert np.array_equal(i[sample], oi), (nq, k, mode)
        assert _bits(s[sample]) == _bits(os_), (nq, k, mode)
    idx.close()


# ---- 13. a view of an index ------------------------------------------------------------------------------------------------
@gpu
@dims
def test_a_view_of_every_other_row(oracle, dim):
    """every other row of an 8 192-row parent with an id_base: the view builds its own fp16 image at the parent's dim; its hits
    carry the parent's ids and equal the oracle over the selected rows"""
    n, nq, base = 8192, 300, 50_000
    corpus, levels, queries = _rows(n, dim, 2400), icd_levels(n, 2401), _rows(nq, dim, 2402)
    rows = np.arange(0, n, 2, dtype=np.int64)
    parent = IcdIndex(corpus, levels, max_nq=nq, max_k=10, id_base=base)
    view = parent.view(rows)
    sub = np.ascontiguousarray(corpus[rows])
    os_, oi = oracle.flat_ip_topk(sub, queries, 10)
    want = oracle.reweight(os_, oi, levels[rows])
    s, i = view.search(queries, 10, MODE_AUTO)
    st = view.stats()
    assert st["last_mode"] == MODE_AUTO and st["fast_path"] == 1 and st["n"] == len(rows) and st["dim"] == dim, st
    assert np.array_equal(i, base + rows[oi]) and _bits(s) == _bits(os_)
    adj, raw, ids, lv = view.search_reweighted(queries, 10, MODE_AUTO)
    assert np.array_equal(ids, base + rows[want[2]]) and _bits(adj) == _bits(want[0]) and _bits(raw) == _bits(want[1])
    assert np.array_equal(lv, want[3])
    view.close()
    st = _check(oracle, parent, corpus, levels, queries, 10, MODE_AUTO, id_base=base)   # the parent is untouched by its view
    assert st["last_mode"] == MODE_AUTO
    parent.close()
