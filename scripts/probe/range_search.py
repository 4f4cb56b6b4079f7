#!/usr/bin/env python3
"""Range search on one MI355X: what a band costs next to the plain exact search.

40 474 x 768 random unit rows (the size of the real ICD-10 corpus), queries = noisy copies of rows, device in / device out,
hipEvents around the call, median of 25 steps after 5 warm-up steps, k = 10. In the SAME run, per batch size:
  (b) the yardstick, existing code: search(mode=MODE_EXACT, k) - the same fp32 products and fused select without a band -
      and, for one query, the plain search (AUTO: the single-launch kernel);
  (a) search_range with range_filter = the score at rank 200 (every hit beyond the top-128), with radius only (the score at
      rank 10: a similarity floor) and the `after` page (cursor = the 10th hit: what an iterator's next() runs).
The one-query rows are also timed from the host (numpy in / numpy out, wall clock): the iterator's time per next().
Prints a report; `> profiles/range_search_probe.log`.
"""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

N, DIM, K = 40474, 768, 10


def main():
    import torch
    from rag_project_icd10_amd._native import MODE_EXACT, IcdIndex
    rng = np.random.default_rng(77)
    corpus = rng.standard_normal((N, DIM), dtype=np.float32)
    corpus /= np.linalg.norm(corpus, axis=1, keepdims=True)
    qb = np.ascontiguousarray(corpus[rng.integers(0, N, 10000)] + 0.1 * rng.standard_normal((10000, DIM), dtype=np.float32), np.float32)
    index = IcdIndex(corpus, rng.integers(1, 4, N).astype(np.int32), max_nq=10000, max_k=128)
    dq = torch.from_numpy(qb).cuda()
    print(f"corpus: {N} x {DIM} random unit rows; device {torch.cuda.get_device_name(0)}; k = {K}")

    def timed(f, steps=25, warm=5):
        for _ in range(warm):
            f()
        ts = []
        for _ in range(steps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
        return statistics.median(ts)

    def host_timed(f, steps=200, warm=20):
        for _ in range(warm):
            f()
        ts = []
        for _ in range(steps):
            t0 = time.perf_counter()
            f()
            ts.append((time.perf_counter() - t0) * 1e6)
        return statistics.median(ts)

    # the bounds, from the ranking itself: scores at ranks 10 and 200 of every query (exact search at k = 128, and k = 128 behind it)
    s128, i128 = index.search(dq, 128, MODE_EXACT)
    s256, _i = index.search_range(dq, 128, after=(s128[:, 127].contiguous(), i128[:, 127].contiguous()), reweighted=False)[:2]
    floor, ceiling = s128[:, 10].contiguous(), s256[:, 200 - 128].contiguous()
    cursor = (s128[:, 9].contiguous(), i128[:, 9].contiguous())
    print("\nnq      (b) exact ms   (a) range_filter@200   (a)/(b)   (a) radius@10   (a)/(b)   (a) after page   (a)/(b)")
    for nq in (10000, 1000, 16, 1):
        q = dq[:nq]
        b = timed(lambda: index.search_reweighted(q, K, MODE_EXACT))
        a1 = timed(lambda: index.search_range(q, K, range_filter=ceiling[:nq]))
        a2 = timed(lambda: index.search_range(q, K, radius=floor[:nq]))
        a3 = timed(lambda: index.search_range(q, K, after=(cursor[0][:nq], cursor[1][:nq])))
        print(f"{nq:<7d} {b:>10.4f}     {a1:>12.4f}         {a1 / b:>6.2f}   {a2:>10.4f}     {a2 / b:>6.2f}   {a3:>10.4f}       {a3 / b:>6.2f}")
    q1 = dq[:1]
    auto = timed(lambda: index.search_reweighted(q1, K))
    print(f"\none query, device in / out: plain search (AUTO) {1e3 * auto:.1f} us")
    # from the host: what MilvusService.search and an iterator's next() pay per call
    hq = qb[:1]
    h_cur = (cursor[0][:1].cpu().numpy(), cursor[1][:1].cpu().numpy())
    h_floor, h_ceil = floor[:1].cpu().numpy(), ceiling[:1].cpu().numpy()
    t_plain = host_timed(lambda: index.search_reweighted(hq, K))
    t_exact = host_timed(lambda: index.search_reweighted(hq, K, MODE_EXACT))
    t_page = host_timed(lambda: index.search_range(hq, K, after=h_cur, reweighted=False))
    t_ceil = host_timed(lambda: index.search_range(hq, K, range_filter=h_ceil))
    t_floor = host_timed(lambda: index.search_range(hq, K, radius=h_floor))
    print(f"one query from the host (numpy in / out, wall clock, median of 200): plain search {t_plain:.1f} us, MODE_EXACT {t_exact:.1f} us, "
          f"iterator page (after) {t_page:.1f} us, range_filter {t_ceil:.1f} us, radius {t_floor:.1f} us")
    t_page128 = host_timed(lambda: index.search_range(hq, 128, after=h_cur, reweighted=False), steps=50, warm=5)
    t_exact128 = host_timed(lambda: index.search(hq, 128, MODE_EXACT), steps=50, warm=5)
    print(f"one query from the host, k = 128: MODE_EXACT {t_exact128:.1f} us, iterator page (after) {t_page128:.1f} us")


if __name__ == "__main__":
    main()
