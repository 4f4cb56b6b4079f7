#!/usr/bin/env python3
"""Embedding-list search on one MI355X: what MAX_SIM over a list of vectors costs.

The corpus and groupings of scripts/probe/grouped_search.py plus every row its own group: 40 474 x 768 random unit rows, vectors =
noisy copies of rows, k = 10, lists of 4 and of 16 vectors at 1, 32 and 512 lists. Device in / device out, hipEvents around the
call, median (min .. max) of 15 steps after 3 warm-up steps, the calls alternating inside every step:
  (a) search_lists (icd_index_search_maxsim), all five outputs;
  (b) search_grouped(scorer="max", group_size=1) on the same vectors: the floor - the two shared kernels and a finish per vector;
  (c) the exact host route: all scores by numpy on the host (one matmul, the per-group maxima, the ordered sums, the top k), wall
      clock, 3 steps, up to 32 lists (512 lists of 16 are 8 192 x 40 474 scores: minutes of matmul for one number).
`--stages`: one search_lists and one grouped search of 512 lists of 16 per grouping and nothing else, for
`rocprofv3 --kernel-trace --stats -- python ...`.
Prints a report; `> profiles/maxsim_search_probe.log`.
"""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from grouped_search import DIM, K, N, groupings  # noqa: E402

SHAPES = ((1, 4), (1, 16), (32, 4), (32, 16), (512, 4), (512, 16))     # (lists, vectors per list)
MAX_VECTORS = 512 * 16


def host_route(corpus, q, T, order, starts, k):
    """all scores on the host, per-group maxima over the (group, row) order, the ordered fp32 sums, the k best groups"""
    S = q @ corpus.T
    best = np.maximum.reduceat(S[:, order], starts, axis=1)
    agg = best[0::T].copy()
    for t in range(1, T):
        agg += best[t::T]
    top = np.argpartition(-agg, min(k, agg.shape[1] - 1), axis=1)[:, :k]
    return np.take_along_axis(agg, top, axis=1)


def main():
    import torch
    from rag_project_icd10_amd._native import IcdIndex
    stages = "--stages" in sys.argv
    rng = np.random.default_rng(77)
    corpus = rng.standard_normal((N, DIM), dtype=np.float32)
    corpus /= np.linalg.norm(corpus, axis=1, keepdims=True)
    qb = np.ascontiguousarray(corpus[rng.integers(0, N, MAX_VECTORS)] + 0.1 * rng.standard_normal((MAX_VECTORS, DIM), dtype=np.float32), np.float32)
    index = IcdIndex(corpus, rng.integers(1, 4, N).astype(np.int32), max_nq=MAX_VECTORS, max_k=128)
    dq = torch.from_numpy(qb).cuda()
    print(f"corpus: {N} x {DIM} random unit rows; device {torch.cuda.get_device_name(0)}; k = {K}")
    made = {}
    for name, g in dict(groupings(rng), identity=np.arange(N)).items():
        grouping = index.grouping(g)
        before = grouping.stats()["bytes"]
        grouping.prepare_scorers(index)
        mid = grouping.stats()["bytes"]
        grouping.prepare_maxsim(index, 512, MAX_VECTORS)
        st = grouping.stats()
        order = np.argsort(g, kind="stable")
        starts = np.flatnonzero(np.r_[True, g[order][1:] != g[order][:-1]])
        made[name] = (grouping, order, starts)
        print(f"grouping {name}: {st['groups']} groups, largest {st['largest_group']} rows, {before / 2**20:.0f} MiB; prepare_maxsim adds "
              f"{(st['bytes'] - mid) / 2**20:.1f} MiB")
    if stages:
        off = np.arange(0, MAX_VECTORS + 1, 16, dtype=np.int64)
        for name, (grouping, _o, _s) in made.items():
            index.search_lists(dq, off, K, grouping)
            index.search_grouped(dq, K, 1, grouping, reweighted=False, scorer="max", group_scores=True)
        torch.cuda.synchronize()
        return

    def timed(calls, steps=15, warm=3):
        """the calls alternate inside every step; -> per call (median, min, max) ms"""
        ts = [[] for _ in calls]
        for step in range(warm + steps):
            for j, f in enumerate(calls):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                f()
                b.record()
                b.synchronize()
                if step >= warm:
                    ts[j].append(a.elapsed_time(b))
        return [(statistics.median(t), min(t), max(t)) for t in ts]

    print("\nlists  T   grouping           (a) search_lists ms (min .. max)   (b) grouped MAX ms (min .. max)    (a)/(b)   (c) host numpy ms")
    for nl, T in SHAPES:
        q, off = dq[:nl * T], np.arange(0, nl * T + 1, T, dtype=np.int64)
        for name, (grouping, order, starts) in made.items():
            (a, alo, ahi), (b, blo, bhi) = timed([
                lambda: index.search_lists(q, off, K, grouping),
                lambda: index.search_grouped(q, K, 1, grouping, reweighted=False, scorer="max", group_scores=True)])
            host = "-"
            if nl <= 32:
                ts = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    host_route(corpus, qb[:nl * T], T, order, starts, K)
                    ts.append((time.perf_counter() - t0) * 1e3)
                host = f"{statistics.median(ts):.1f}"
            print(f"{nl:<6d} {T:<3d} {name:<18s} {a:>8.3f} ({alo:.3f} .. {ahi:.3f})         {b:>8.3f} ({blo:.3f} .. {bhi:.3f})       {a / b:>6.2f}    {host:>8s}")


if __name__ == "__main__":
    main()
