"""Searches over row shards of several GiB (run with -m gpu on an MI355X): 10 M x 768 (BASELINE configs[4] on one GPU),
5 M x 768 with an id base past 2^32, 7 M x 1024 and a view of every other row of the 10 M shard.

At these sizes the coarse pass's lists, limited by the corpus alone, would run past the reach of the kernel's per-list
buffer descriptor (2^31 - 1 bytes, a 32-bit tile offset); the list planner caps them (flat_partition.hpp
plan_coarse_lists, tests/test_flat_partition.py). Every query of every batch is checked against the CPU oracle bit for bit
(ids; raw, adjusted scores and levels), the way test_gpu_parity._check does.

Reference without sweeping 10 M rows per query on the CPU: a float64 GEMM on the device is a filter. With T a query's
k-th float64 score, e32 = gamma_dim(2^-24) |q| max|c| (the oracle's fmaf chain) and e64 = gamma_dim(2^-53) |q| max|c| (the
float64 GEMM, any order), every row of the oracle's top-k (ties included) has a float64 score >= T - 2 (e32 + e64). The
oracle runs on those rows only (in row order, so that its id tie-break is the global one); the top-k of the largest k is
computed once and its prefixes serve the smaller k.

The data: unit Gaussian rows made on the device, a few thousand exact duplicate row pairs half the shard apart (the id
tie-break at scale), queries that are noisy copies of rows spread over the shard, the duplicated rows among them.
"""
import time

import numpy as np
import pytest

from conftest import icd_levels
from test_flat_partition import build_checker, coarse_plan

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from rag_project_icd10_amd._native import MODE_AUTO, MODE_EXACT, IcdIndex  # noqa: E402

NQ = 16384
MARGIN_ROWS = 64             # candidates beyond k the filter may keep
_used = {"peak_gb": 0.0}


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _note_memory():
    free, total = torch.cuda.mem_get_info()
    _used["peak_gb"] = max(_used["peak_gb"], (total - free) / 2 ** 30)


def _shard(n, dim, seed):
    """unit Gaussian rows on the device; every 1 365th row of the first half (a few thousand) copied half the shard further on;
    queries: noisy copies of NQ rows spread evenly over the shard (every 8th one a duplicated row)"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    rows = torch.randn((n, dim), generator=g, device="cuda", dtype=torch.float32)
    rows /= rows.norm(dim=1, keepdim=True)
    src = torch.arange(0, n // 2, 1365, device="cuda")
    rows[src + n // 2] = rows[src]
    pick = torch.linspace(0, n - 1, NQ, device="cuda").round().long()
    pick[::8] = src[torch.arange(0, NQ, 8, device="cuda") % src.numel()]
    q = rows[pick] + 0.3 * torch.randn((NQ, dim), generator=g, device="cuda", dtype=torch.float32) / dim ** 0.5
    q /= q.norm(dim=1, keepdim=True)
    return rows, q.contiguous(), int(src.numel())


def _reference(oracle, rows, queries, kmax, ks):
    """the oracle's top-kmax of every query over all rows (local row indices), via the float64 filter; asserts that for
    every k in ks the filter keeps at most k + MARGIN_ROWS rows"""
    n, dim = rows.shape
    nq = queries.shape[0]
    m = kmax + MARGIN_ROWS + 1
    q64 = queries.double()
    cmax = float(rows.norm(dim=1).max()) * (1 + 1e-5)   # (an fp32 norm: rounded up past its own error)

    def gamma(u):
        return dim * u / (1 - dim * u)
    margin = 2 * (gamma(2.0 ** -24) + gamma(2.0 ** -53)) * q64.norm(dim=1) * cmax
    topv = torch.full((nq, m), -float("inf"), dtype=torch.float64, device="cuda")
    topi = torch.zeros((nq, m), dtype=torch.int64, device="cuda")
    rc = 1 << 19
    qc = max(1, min(nq, (10 << 30) // (rc * 8) // 2))         # one float64 score chunk <= 5 GB
    for r0 in range(0, n, rc):
        c64 = rows[r0:r0 + rc].double()
        for q0 in range(0, nq, qc):
            s = q64[q0:q0 + qc] @ c64.T
            v, i = s.topk(min(m, s.shape[1]), dim=1)
            v = torch.cat([topv[q0:q0 + qc], v], 1)
            i = torch.cat([topi[q0:q0 + qc], i + r0], 1)
            v, j = v.topk(m, dim=1)
            topv[q0:q0 + qc], topi[q0:q0 + qc] = v, i.gather(1, j)
            del s
        del c64
        _note_memory()
    keep = {}
    for k in ks:
        thr = topv[:, k - 1] - margin
        cnt = (topv >= thr[:, None]).sum(1)
        assert int(cnt.max()) <= k + MARGIN_ROWS, f"the float64 filter keeps {int(cnt.max())} rows at k = {k}"
        keep[k] = cnt
    cnt = keep[kmax].cpu().numpy()
    order_i = topi.cpu().numpy()
    qh = queries.cpu().numpy()
    ref_s = np.empty((nq, kmax), np.float32)
    ref_i = np.empty((nq, kmax), np.int64)
    for q0 in range(0, nq, 2048):
        q1 = min(nq, q0 + 2048)
        c = int(cnt[q0:q1].max())
        cand = np.sort(order_i[q0:q1, :c], axis=1)     # (rows past a query's own count are filtered out below)
        g = rows[torch.from_numpy(cand).cuda()].cpu().numpy()
        for qi in range(q0, q1):
            own = np.sort(order_i[qi, :cnt[qi]])
            at = np.searchsorted(cand[qi - q0], own)
            s, i = oracle.flat_ip_topk(g[qi - q0, at], qh[qi], kmax, nthreads=1)
            ref_s[qi], ref_i[qi] = s[0], own[i[0]]
    return ref_s, ref_i


def _check(oracle, index, queries, ref_s, ref_i, k, mode, levels, id_of, id_base):
    """every query: ids exact, raw / adjusted scores and levels bit for bit against the oracle's top-k"""
    nq = queries.shape[0]
    adj, raw, ids, lv = (t.cpu().numpy() for t in index.search_reweighted(queries, k, mode))
    oi = id_of(ref_i[:nq, :k])
    want = oracle.reweight(np.ascontiguousarray(ref_s[:nq, :k]), oi, levels, id_base=id_base)
    bad = np.nonzero((ids != want[2]).any(1))[0]
    assert bad.size == 0, f"k={k} nq={nq} mode={mode}: {bad.size} queries with other ids, first {bad[:5]}"
    assert _bits(raw) == _bits(want[1]) and _bits(adj) == _bits(want[0]) and np.array_equal(lv, want[3])
    return index.stats()


def _assert_plan_capped(exe, n, dim, k, over_bytes):
    """the planner's plan for this shape: the uncapped lists run past over_bytes, the capped ones stay in reach"""
    free = coarse_plan(exe, n, dim, NQ, k, max_list_tiles=-1)
    capped = coarse_plan(exe, n, dim, NQ, k)
    assert free["longest_list_bytes"] > over_bytes and free["in_reach"] == 0, free
    assert capped["ok"] and capped["in_reach"] and capped["list_tiles"] == capped["max_list_tiles"] < free["list_tiles"], capped


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return build_checker(tmp_path_factory.mktemp("plan"))


def _report(name, t0):
    _note_memory()
    print(f"\n[{name}] {time.time() - t0:.1f} s, device memory peak so far {_used['peak_gb']:.1f} GiB")


def test_10m_rows_768(oracle, checker):
    """BASELINE configs[4] on one GPU: 10 M x 768, 16 384 queries at k = 1, 10, 32, 100 (AUTO); the same index at 1, 2, 9
    and 16 queries (single-launch and streaming kernels); EXACT at 300 queries, k = 10 and 64; k = 128; then a view of
    every other row."""
    t0 = time.time()
    n, dim = 10_000_000, 768
    for k in (1, 10):
        _assert_plan_capped(checker, n, dim, k, 4 << 30)
    rows, q, _ = _shard(n, dim, 101)
    levels = icd_levels(n, 102)
    index = IcdIndex(rows, levels, max_nq=NQ, max_k=128)
    _note_memory()
    ref_s, ref_i = _reference(oracle, rows, q, 100, (1, 10, 32, 100))
    for k in (1, 10, 32, 100):
        st = _check(oracle, index, q, ref_s, ref_i, k, MODE_AUTO, levels, lambda i: i, 0)
        assert st["last_mode"] == MODE_AUTO
        if k <= 10:
            assert st["last_fallback"] <= 20, st
    for nq in (1, 2, 9, 16):
        _check(oracle, index, q[:nq], ref_s, ref_i, 10, MODE_AUTO, levels, lambda i: i, 0)
    for k in (10, 64):
        _check(oracle, index, q[:300], ref_s, ref_i, k, MODE_EXACT, levels, lambda i: i, 0)
    s128, i128 = _reference(oracle, rows, q[:300], 128, (128,))
    _check(oracle, index, q[:300], s128, i128, 128, MODE_AUTO, levels, lambda i: i, 0)
    _report("10M x 768", t0)
    # a view of every other row: hits carry the parent's ids
    _assert_plan_capped(checker, n // 2, dim, 10, 2 << 30)
    view = index.view(torch.arange(0, n, 2, device="cuda"), max_nq=NQ, max_k=10)
    index.close()
    half = rows[::2].contiguous()
    del rows
    vs, vi = _reference(oracle, half, q, 10, (10,))
    del half
    st = _check(oracle, view, q, vs, vi, 10, MODE_AUTO, levels, lambda i: 2 * i, 0)
    assert st["last_mode"] == MODE_AUTO
    view.close()
    _report("view of 5M rows", t0)


def test_5m_rows_id_base_past_2_32(oracle, checker):
    t0 = time.time()
    n, dim, base = 5_000_000, 768, (1 << 32) + 12_345
    _assert_plan_capped(checker, n, dim, 10, 2 << 30)
    rows, q, _ = _shard(n, dim, 202)
    levels = icd_levels(n, 203)
    index = IcdIndex(rows, levels, max_nq=NQ, max_k=10, id_base=base)
    ref_s, ref_i = _reference(oracle, rows, q, 10, (10,))
    del rows
    st = _check(oracle, index, q, ref_s, ref_i, 10, MODE_AUTO, levels, lambda i: i + base, base)
    assert st["last_mode"] == MODE_AUTO and st["last_fallback"] <= 20, st
    index.close()
    _report("5M x 768, id base 2^32 + 12 345", t0)


def test_7m_rows_1024(oracle, checker):
    t0 = time.time()
    n, dim = 7_000_000, 1024
    _assert_plan_capped(checker, n, dim, 10, 4 << 30)
    rows, q, _ = _shard(n, dim, 303)
    levels = icd_levels(n, 304)
    index = IcdIndex(rows, levels, max_nq=NQ, max_k=10)
    ref_s, ref_i = _reference(oracle, rows, q, 10, (10,))
    del rows
    st = _check(oracle, index, q, ref_s, ref_i, 10, MODE_AUTO, levels, lambda i: i, 0)
    assert st["last_mode"] == MODE_AUTO and st["last_fallback"] <= 20, st
    index.close()
    _report("7M x 1024", t0)
