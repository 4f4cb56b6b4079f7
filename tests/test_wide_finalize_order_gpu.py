"""The wide-window finalize of a family-shaped corpus in FAMILY ORDER, off the one batch shape it was tested at.

An index in wide mode answers a batch of 2 048+ queries at k <= 32 with ONE finalize over every query, widest window, and
(icd_search.hip auto_first_finalize) visits the queries family by family: order_keys_kernel / order_scatter_kernel (finalize.hpp)
counting-sort them by the row bucket of their best coarse candidate, order_slot deals four consecutive positions of that order to
one work-group and consecutive work-groups of it to one XCD, the slots behind the batch in the last work-group hold -1, and
finalize_kernel<true, false, 4> runs with qlist = order, lists_by_query = 1 and nq rounded up to a multiple of 4. The two tests that
reached this (test_gpu_parity.py::test_family_corpus_is_certified_within_the_call, one case of test_certified_dim1024_gpu.py) ran
10 000 and 2 049 queries: no padding at the first, one `nblk % 8`, shift = 6, family_order never compared with its off switch, the
narrow re-probe of every 64th large search never reached.

Data: test_gpu_parity._tight_family_corpus, dim 768, spread 0.10, 124 rows per family, levels from icd_levels. FAMILIES = 100
(12 400 rows, the size test_second_pass_switch_and_gaussian_batches_skip_it uses) is where the search for a size started and where
it ended: both the create-time probe and, with probe=False, one narrow batch of 2 048 put the index into wide mode there (measured
on an MI355X; the figures are in DESIGN.md section 30), so the count was never grown. Case 3 needs 530 families (65 720 rows:
n >> 6 = 1 026 >= ORDER_BUCKETS) by construction; case 7 runs dim 1024 at the same 100 families.

Every compared call asserts from stats() that the path ran (_assert_wide_path) and compares ALL queries, bytes-equal, with the same
index searched in MODE_EXACT, and a sample (query 0, the last four, every 16th in between) with oracle.flat_ip_topk +
oracle.reweight. The batch of every call is permuted with a fresh seeded permutation and the result un-permuted (_Wide.search): a
slot that finalize never visits leaves its output rows unwritten, torch's caching allocator hands the next call the block the
previous one filled, and with the same query order the stale bytes ARE the right answer. For the same reason the returned
tensors are overwritten once they have been read.

Not tested: the bucket skew. A wrong `shift` or bucket only moves work between XCDs and changes no result.
"""
import numpy as np
import pytest

from conftest import icd_levels, unit_rows
from test_gpu_parity import _tight_family_corpus

from rag_project_icd10_amd._native import MODE_AUTO, MODE_EXACT, IcdIndex  # noqa: E402

pytestmark = pytest.mark.gpu

FAMILIES, PER, SPREAD = 100, 124, 0.10
POOL = 4099                # queries generated per corpus: the largest batch; smaller batches are its first nq
CO_KP = 16                 # candidates per list (coarse_common.hpp)
WIDE_MIN_NQ = 2048         # search_policy.hpp
WIDE_REPROBE = 64          # search_policy.hpp: every 64th large search in wide mode runs narrow again
NAMES = ("adjusted", "raw", "ids", "levels")


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _sample(nq, step=16):
    return np.unique(np.concatenate([np.arange(0, nq, step), np.arange(max(nq - 4, 0), nq)]))


class _Family:
    """one corpus, its levels and its query pool, on the host (read-only) and on the device"""

    def __init__(self, nfam, dim, seed, id_base=0, pool=POOL):
        import torch
        self.corpus, self.queries = _tight_family_corpus(nfam, PER, dim, SPREAD, pool, seed)
        self.levels = icd_levels(len(self.corpus), seed + 1)
        self.id_base = id_base
        self.dcorpus = torch.from_numpy(self.corpus).cuda()
        self.dqueries = torch.from_numpy(self.queries).cuda()
        for a in (self.corpus, self.queries, self.levels):
            a.setflags(write=False)
        self._want = {}    # k -> the oracle's answers for the pool's queries, filled row by row as samples ask for them

    def oracle_rows(self, oracle, k, rows):
        """oracle.flat_ip_topk + oracle.reweight of the pool's queries `rows`: each computed once per k, then shared"""
        if k not in self._want:
            nq = len(self.queries)
            self._want[k] = (np.zeros(nq, bool), [np.empty((nq, k), dt) for dt in (np.float64, np.float32, np.int64, np.int32)])
        have, want = self._want[k]
        todo = rows[~have[rows]]
        if len(todo):
            for w, o in zip(want, _oracle(oracle, self, self.queries[todo], k)):
                w[todo] = o
            have[todo] = True
        return [w[rows] for w in want]


def _oracle(oracle, fam, queries, k):
    s, i = oracle.flat_ip_topk(fam.corpus, queries, k, id_base=fam.id_base)
    return oracle.reweight(s, i, fam.levels, id_base=fam.id_base)


@pytest.fixture(scope="module")
def fam():
    return _Family(FAMILIES, 768, 3000)


def _assert_wide_path(st, nq):
    """what stats() shows of a search that took the wide-window finalize (auto_first_finalize's wide_fin) and nothing behind it"""
    assert st["last_mode"] == MODE_AUTO and st["last_nq"] == nq, st
    assert st["wide_mode"] == 1, st
    assert st["last_second_pass_lists"] == 0, st
    assert st["last_chunks"] * CO_KP >= 128, st                 # pc * KP >= 128
    assert st["last_fallback"] <= 0.01 * nq, st                 # the bound of test_family_corpus_is_certified_within_the_call


class _Wide:
    """An index over `fam` that is in wide mode, by the create-time probe or (probe=False) by one narrow large batch whose
    counters the next search judges (search_policy.hpp). That next search is the MODE_EXACT reference of the test: before
    policy_unplanned_search it overwrote the narrow batch's counters with its own zeros and the index stayed narrow."""

    def __init__(self, fam, probe, max_nq, max_k=32, seed=0):
        self.fam, self.seed, self.calls = fam, seed, 0
        self.idx = IcdIndex(fam.dcorpus, fam.levels, max_nq=max_nq, max_k=max_k, id_base=fam.id_base, probe=probe)
        st = self.idx.stats()
        if probe:
            assert st["wide_mode"] == 1 and st["last_nq"] == 0, st
        else:
            assert st["wide_mode"] == 0, st
            self.idx.search_reweighted(fam.dqueries[:WIDE_MIN_NQ], 10)
            st = self.idx.stats()           # (waits for the search: the next one finds its counters)
            print(f"narrow batch without the probe: second pass for {st['last_second_pass']} of {WIDE_MIN_NQ} ({st['last_second_pass_lists']} lists), "
                  f"exact re-search for {st['last_fallback']}")
            assert st["wide_mode"] == 0 and st["last_second_pass_lists"] > 0, st

    def close(self):
        self.idx.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def exact(self, dq, k):
        """MODE_EXACT on this index, batch order: the reference for ALL queries"""
        out = [t.cpu().numpy() for t in self.idx.search_reweighted(dq, k, MODE_EXACT)]
        assert self.idx.stats()["last_mode"] == MODE_EXACT
        return out

    def search(self, dq, k, on_device=False):
        """One AUTO call on a freshly permuted batch -> (the outputs in batch order, stats).
        No two calls of an index share a query order: a slot that finalize never visits leaves its output rows unwritten, and the
        caching allocator hands this call the block the previous call filled - with the same order those stale bytes are the right
        answer and a dropped slot passes. The outputs are overwritten once read, so the block comes back holding no answer at all."""
        import torch
        nq = dq.shape[0]
        self.calls += 1
        perm = torch.from_numpy(np.random.default_rng([self.seed, self.calls]).permutation(nq)).cuda()
        out = self.idx.search_reweighted(dq[perm], k, MODE_AUTO)
        st = self.idx.stats()
        got = []
        for t in out:
            u = torch.empty_like(t)
            u[perm] = t
            got.append(u if on_device else u.cpu().numpy())
            t.view(torch.uint8).fill_(0xA5)
        return got, st


def _equal_all(got, ref, what):
    for name, g, r in zip(NAMES, got, ref):
        if _bits(g) != _bits(r):
            bad = np.nonzero((np.ascontiguousarray(g).view(np.uint8).reshape(len(g), -1) != np.ascontiguousarray(r).view(np.uint8).reshape(len(r), -1)).any(1))[0]
            raise AssertionError(f"{what}: {name} of {len(bad)} of {len(g)} queries differ, first {bad[:8]}")


def _compare(oracle, w, dq, k, exact, want, rows, what, wide=True):
    """one compared call: the path from stats(), ALL queries against MODE_EXACT, the sample `rows` against the oracle's `want`"""
    got, st = w.search(dq, k)
    print(f"{what}: lists {st['last_chunks']} second-pass lists {st['last_second_pass_lists']} exact re-search {st['last_fallback']} wide {st['wide_mode']}")
    if wide:
        _assert_wide_path(st, dq.shape[0])
    _equal_all(got, exact, f"{what} against MODE_EXACT")
    _equal_all([g[rows] for g in got], want, f"{what} against the oracle")
    return got, st


def _compare_pool(oracle, w, nq, k, what, exact=None, step=16, wide=True):
    """a compared call on the first nq queries of the corpus's pool"""
    dq = w.fam.dqueries[:nq]
    exact = exact if exact is not None else w.exact(dq, k)
    rows = _sample(nq, step)
    return _compare(oracle, w, dq, k, exact, w.fam.oracle_rows(oracle, k, rows), rows, what, wide)


# ---- 1. ragged batches -----------------------------------------------------------------------------------------------------
# padding 0, 3, 2, 1; nblk = ceil(nq / 4) = 512, 513, 513, 513, 513, 520, 751, 1 025: nblk % 8 = 0, 1, 1, 1, 1, 0, 7, 1; the scatter
# kernel's second work-group holds 0, 1, 2, 3, 4, 32 queries, its third 953 of 3 001, its fifth 3 of 4 099
RAGGED = [(2048, (10,)), (2049, (1, 10, 32)), (2050, (10,)), (2051, (10,)), (2052, (10,)), (2080, (10,)), (3001, (1, 10, 32)), (4099, (10,))]


@pytest.mark.parametrize("probe", [True, False], ids=["probe", "narrow-batch"])
@pytest.mark.parametrize("nq,ks", RAGGED, ids=[str(nq) for nq, _ in RAGGED])
def test_ragged_batches(oracle, fam, nq, ks, probe):
    with _Wide(fam, probe, max_nq=nq, seed=nq) as w:
        for k in ks:
            _compare_pool(oracle, w, nq, k, f"nq {nq} k {k} {'probe' if probe else 'narrow batch'}")


def test_k33_is_the_other_side_of_the_gate(oracle, fam):
    """policy_decide plans wide only at k <= 32: on an index in wide mode (shown by a k = 32 call first) a k = 33 batch runs the
    narrow plan - fewer lists, a second pass planned behind it, no wide-window-first finalize - and is exact. (Its counters may take
    the index out of wide mode, policy_take_counters: it is the last call of its index.)"""
    nq = 2049
    with _Wide(fam, True, max_nq=nq, max_k=33, seed=33) as w:
        _, st32 = _compare_pool(oracle, w, nq, 32, "nq 2049 k 32")
        _, st33 = _compare_pool(oracle, w, nq, 33, "nq 2049 k 33", wide=False)
        assert st33["last_mode"] == MODE_AUTO and st33["last_nq"] == nq, st33
        assert st33["last_chunks"] < st32["last_chunks"] and st33["last_second_pass_lists"] > 0, (st32, st33)


# ---- 2. the option off equals the option on --------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", [2051, 4099])
def test_family_order_off_equals_on(oracle, fam, nq):
    """ICD_OPT_FAMILY_ORDER = 0 runs the same finalize in batch order (no qlist, nq as it is): both settings against both
    references and against each other. The option-off half runs first: a failure that names family_order 1 has passed it."""
    with _Wide(fam, False, max_nq=nq, seed=7 * nq) as w:
        exact = w.exact(fam.dqueries[:nq], 10)
        try:
            w.idx.set_option("family_order", 0)
            off, _ = _compare_pool(oracle, w, nq, 10, f"nq {nq} family_order 0", exact)
            w.idx.set_option("family_order", 1)
            on, _ = _compare_pool(oracle, w, nq, 10, f"nq {nq} family_order 1", exact)
        finally:
            w.idx.set_option("family_order", 1)
        _equal_all(on, off, f"nq {nq} family_order 1 against 0")


# ---- 3. shift > 6 ------------------------------------------------------------------------------------------------------------
def test_more_rows_than_the_buckets_hold_at_shift_6(oracle):
    """530 families = 65 720 rows: n >> 6 = 1 026 >= ORDER_BUCKETS, auto_first_finalize raises shift to 7; id_base 2^32 + 1. The
    oracle's sample is query 0, the last four and every 256th (the CPU cost is the corpus)."""
    big = _Family(530, 768, 3100, id_base=2 ** 32 + 1, pool=2051)
    assert (len(big.corpus) >> 6) >= 1024 and (len(big.corpus) >> 7) < 1024
    with _Wide(big, True, max_nq=2051, max_k=10, seed=3) as w:
        got, _ = _compare_pool(oracle, w, 2051, 10, "65 720 rows nq 2051", step=256)
    assert got[2].min() >= big.id_base and got[2].max() < big.id_base + len(big.corpus)


# ---- 4. queries that are not family members ----------------------------------------------------------------------------------
def test_family_gaussian_and_copied_row_queries_interleaved(oracle, fam):
    """2 049 queries in three interleaved thirds: family queries, Gaussian unit queries, exact copies of corpus rows of eight
    families (rows 0 .. 991: at shift 6 sixteen of the 194 buckets get a third of the batch, most buckets of the Gaussian and family
    thirds a handful)"""
    import torch
    nq = 2049
    q = np.empty((nq, 768), np.float32)
    q[0::3] = fam.queries[:683]
    q[1::3] = unit_rows(683, 768, 3201)
    q[2::3] = fam.corpus[np.random.default_rng(3202).integers(0, 8 * PER, 683)]
    dq = torch.from_numpy(q).cuda()
    rows = _sample(nq)
    with _Wide(fam, True, max_nq=nq, max_k=10, seed=4) as w:
        got, _ = _compare(oracle, w, dq, 10, w.exact(dq, 10), _oracle(oracle, fam, q[rows], 10), rows, "three kinds of queries")
    assert (got[1][2::3].max(1) > 0.9999).all()      # (a copied row finds itself)


# ---- 5. unusable queries -------------------------------------------------------------------------------------------------------
def test_zero_and_nan_queries_are_filed_under_bucket_0(oracle, fam):
    """2 050 queries, the first and the last all zeros, query 1 024 holding a NaN: order_keys_kernel finds no candidate for them
    (best == 0) and files them under bucket 0; finalize cannot certify them and the exact re-search answers. The oracle defines both:
    all scores of a zero query tie at 0 (rows by id), a NaN query has no hit (id -1, -inf, level 0) - 0, 1 024 and 2 049 are in the
    sample, so the three are compared with MODE_EXACT and with the oracle like every other query."""
    import torch
    nq = 2050
    q = fam.queries[:nq].copy()
    q[0] = 0.0
    q[-1] = 0.0
    q[1024, 5] = np.nan
    rows = _sample(nq)
    assert {0, 1024, nq - 1} <= set(rows.tolist())
    dq = torch.from_numpy(q).cuda()
    with _Wide(fam, False, max_nq=nq, max_k=10, seed=5) as w:
        got, st = _compare(oracle, w, dq, 10, w.exact(dq, 10), _oracle(oracle, fam, q[rows], 10), rows, "zero and NaN queries")
    assert st["last_fallback"] >= 3, st
    assert (got[2][1024] == -1).all() and (got[2][0] == np.arange(10)).all() and (got[2][-1] == np.arange(10)).all()


# ---- 6. the re-probe -----------------------------------------------------------------------------------------------------------
def test_every_64th_large_search_probes_narrow_and_returns_to_wide_mode(fam):
    """130 searches of 2 048 queries on one wide-mode index, each on its own permutation, all queries against MODE_EXACT (computed
    once). policy_decide runs every WIDE_REPROBE-th of them on the narrow plan with the second pass behind it; on this corpus that
    pass has nearly every query to take in, so policy_take_counters keeps wide_mode (it leaves only when the narrow first finalize
    flagged <= 5 % of the batch) and the search after a re-probe is wide again. Compared on the device, by bits."""
    import torch
    nq, k = WIDE_MIN_NQ, 10
    dq = fam.dqueries[:nq]
    as_bits = {torch.float64: torch.int64, torch.float32: torch.int32}
    with _Wide(fam, True, max_nq=nq, max_k=k, seed=6) as w:
        exact = [t.view(as_bits.get(t.dtype, t.dtype)) for t in w.idx.search_reweighted(dq, k, MODE_EXACT)]
        assert w.idx.stats()["last_mode"] == MODE_EXACT
        narrow = []
        for i in range(130):
            got, st = w.search(dq, k, on_device=True)
            for name, g, e in zip(NAMES, got, exact):
                assert torch.equal(g.view(e.dtype), e), f"search {i}: {name} differ from MODE_EXACT"
            if st["last_second_pass_lists"] > 0:
                narrow.append(i)
                assert st["last_mode"] == MODE_AUTO and st["last_chunks"] * CO_KP < 320, st   # (the narrow plan: PASS2_BELOW)
                if len(narrow) == 2:
                    # behind the SECOND re-probe, before the next large batch: a MODE_EXACT batch and a one-query call, which leave
                    # counters of their own (nothing flagged). The verdict on the re-probe is taken from the narrow search's all
                    # the same (policy_unplanned_search): read as the re-probe's, those said "all certified" and the index left
                    # wide mode until the next narrow batch
                    w.idx.search_reweighted(dq[:300], k, MODE_EXACT)
                    w.idx.search_reweighted(dq[:1], k, MODE_AUTO)
                    assert w.idx.stats()["wide_mode"] == 1
            else:
                _assert_wide_path(st, nq)
            if narrow and narrow[-1] == i - 1:
                assert st["wide_mode"] == 1 and st["last_second_pass_lists"] == 0, (i, st)
        print(f"narrow re-probes at searches {narrow}")
        assert narrow == [WIDE_REPROBE - 1, 2 * WIDE_REPROBE - 1], narrow


# ---- 7. dim 1024 ---------------------------------------------------------------------------------------------------------------
def test_dim_1024(oracle):
    """launch_finalize_t<true, false, 4> behind the family order at the other certified dim: 100 families, 2 051 queries"""
    wide = _Family(FAMILIES, 1024, 3300, pool=2051)
    with _Wide(wide, True, max_nq=2051, max_k=10, seed=7) as w:
        _compare_pool(oracle, w, 2051, 10, "dim 1024 nq 2051")
