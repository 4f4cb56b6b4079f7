"""Probe of the wide search, one MI355X, through the ctypes layer. Corpus: 40 474 x 768 random unit rows (the
size of the ICD-10 corpus). For nq in {1, 40, 1 000} and k in {1 000, 4 096, 16 384}, device queries in and device tensors out,
the device span between two events around the call, median of STEPS after WARMUP warm-up steps, the routes alternating inside
each step:
  (a) wide     IcdWide(index).search_wide(queries, k, reweighted=False): one sweep, the radix threshold, the collect, the sort
  (b) paging   the route without it: ceil(k / 128) calls of search_range(k = 128) whose `after` cursor is the last hit of the page
               before (the cursor stays on the device here; services/range_search.py passes it through the host)
  (c) host     every score of every query pulled to the host (an fp32 matmul on the device, one copy), numpy.argpartition and
               a sort of the k best - wall time, the host part included; BLAS sums, not the canonical chain
The ids of (a) and (b) are compared first (0 differences expected: both are exact).
The per-kernel split of (a) is not taken here: it needs a kernel trace in a run of its own.
Usage: python scripts/probe/wide_search.py > profiles/wide_search_probe.log"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

N, DIM = 40474, 768
STEPS, WARMUP = 7, 2


def span(fn):
    """device milliseconds between two events around fn()"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    from rag_project_icd10_amd import _native
    rng = np.random.default_rng(0)
    corpus = rng.standard_normal((N, DIM), dtype=np.float32)
    corpus /= np.linalg.norm(corpus, axis=1, keepdims=True)
    index = _native.IcdIndex(corpus, None, device=0, max_nq=1024, max_k=128)
    dcorpus = torch.from_numpy(corpus).cuda()
    ws = _native.IcdWide(index, 1000)
    print(f"wide search probe: n={N} dim={DIM} steps={STEPS} warmup={WARMUP} workspace {ws.stats()}", flush=True)
    print("nq k | (a) wide ms | (b) paging ms (pages) | (c) host ms | (b)/(a) (c)/(a)", flush=True)
    for nq in (1, 40, 1000):
        q = rng.standard_normal((nq, DIM), dtype=np.float32)
        q /= np.linalg.norm(q, axis=1, keepdims=True)
        dq = torch.from_numpy(q).cuda()
        for k in (1000, 4096, 16384):
            pages = (k + 127) // 128

            def route_a():
                return ws.search_wide(dq, k, reweighted=False)

            def route_b():
                ids, after = [], None
                for _ in range(pages):
                    raw, pid, _lv = index.search_range(dq, 128, after=after, reweighted=False)
                    ids.append(pid)
                    after = (raw[:, -1].contiguous(), pid[:, -1].contiguous())
                return torch.cat(ids, dim=1)[:, :k]

            def route_c():
                sc = (dq @ dcorpus.T).cpu().numpy()
                part = np.argpartition(-sc, k - 1, axis=1)[:, :k]
                order = np.argsort(-np.take_along_axis(sc, part, axis=1), axis=1, kind="stable")
                return np.take_along_axis(part, order, axis=1)

            got_a, got_b = route_a()[2].cpu().numpy(), route_b().cpu().numpy()
            diff = int((got_a != got_b).sum())
            ta, tb, tc = [], [], []
            for step in range(WARMUP + STEPS):
                a_ms, b_ms, c_ms = span(route_a)[0], span(route_b)[0], wall(route_c)[0]
                if step >= WARMUP:
                    ta.append(a_ms), tb.append(b_ms), tc.append(c_ms)
            a, b, c = np.median(ta), np.median(tb), np.median(tc)
            print(f"{nq:5d} {k:6d} | {a:9.3f} (min {min(ta):.3f} max {max(ta):.3f}) | {b:9.3f} ({pages}) | {c:9.3f} | {b / a:6.2f} {c / a:6.2f} | ids differing from paging: {diff}", flush=True)
    ws.close()
    index.close()


if __name__ == "__main__":
    main()
