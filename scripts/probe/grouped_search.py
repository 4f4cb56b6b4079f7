#!/usr/bin/env python3
"""Grouping search on one MI355X: what `group_by_field` costs.

40 474 x 768 random unit rows (the size of the real ICD-10 corpus), queries = noisy copies of rows, device in / device out,
hipEvents around the call, median of 25 steps after 5 warm-up steps. Groupings shaped like the real columns: `parent_code`-like
(9 726 groups, one of 5 031 rows), `category`-like (2 000 groups of ~20 consecutive rows), `level`-like (3 groups of
23 337 / 12 106 / 5 031 rows, scattered). Reported per (queries, grouping, group_size) at k = 10:
  (a) the grouped search;
  (b) search(mode=MODE_EXACT, k=10) on the same box in the same run - the same fp32 products with a fused select: the yardstick;
  (c) search(k=128) + de-duplication by group on the host (device time of the search alone), with the share of queries it answers
      wrongly (fewer than k groups in the top-128, or another set of rows than the exact answer).
Grouping creation (host ordering + upload + workspace) is timed separately.
`--stages`: one grouped search of 10 000 queries per grouping and nothing else, for `rocprofv3 --kernel-trace --stats -- python ...`.
Prints a report; `> profiles/grouped_search_probe.log`.
"""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

N, DIM, K = 40474, 768, 10


def groupings(rng):
    parent = np.empty(N, np.int64)
    parent[:5031] = 0                                          # the level-1 rows: no parent, one group
    parent[5031:] = 1 + np.sort(rng.integers(0, 9725, N - 5031))
    level = np.zeros(N, np.int64)
    perm = rng.permutation(N)
    level[perm[23337:23337 + 12106]] = 1
    level[perm[23337 + 12106:]] = 2
    return {"parent_code-like": parent, "category-like": np.arange(N) * 2000 // N, "level-like": level}


def main():
    import torch
    from rag_project_icd10_amd._native import MODE_EXACT, IcdIndex
    stages = "--stages" in sys.argv
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

    made = {}
    for name, g in groupings(rng).items():
        t0 = time.perf_counter()
        made[name] = (g, index.grouping(g))
        ms = (time.perf_counter() - t0) * 1e3
        st = made[name][1].stats()
        print(f"grouping {name}: {st['groups']} groups, largest {st['largest_group']} rows, {st['bytes'] / 2**20:.0f} MiB "
              f"(workspace for 10 000-query calls), created in {ms:.1f} ms")
    if stages:
        for name, (g, grouping) in made.items():
            for s in (1, 3):
                index.search_grouped(dq, K, s, grouping)
        torch.cuda.synchronize()
        return
    print("\nnq      grouping           s   (a) grouped ms   (b) exact k=10 ms   (a)/(b)   (c) k=128 ms   (c) wrong")
    for nq in (10000, 1000, 16, 1):
        q = dq[:nq]
        b = timed(lambda: index.search(q, K, MODE_EXACT))
        c = timed(lambda: index.search(q, 128))
        _s128, i128 = index.search(q, 128)
        i128 = i128.cpu().numpy()
        for name, (g, grouping) in made.items():
            for s in (1, 3):
                a = timed(lambda: index.search_grouped(q, K, s, grouping))
                _r, ids, _l, _g = (t.cpu().numpy() for t in index.search_grouped(q, K, s, grouping, reweighted=False))
                wrong = 0
                for qi in range(nq):   # the host de-duplication of a top-128
                    seen = {}
                    for row in i128[qi]:
                        seen.setdefault(int(g[row]), []).append(int(row))
                    dedup = [r for grp in list(seen)[:K] for r in seen[grp][:s]]
                    wrong += dedup != [int(r) for r in ids[qi] if r >= 0]
                print(f"{nq:<7d} {name:<18s} {s:<3d} {a:>10.3f}       {b:>10.3f}          {a / b:>6.2f}    {c:>9.3f}      {100.0 * wrong / nq:6.1f} %")


if __name__ == "__main__":
    main()
