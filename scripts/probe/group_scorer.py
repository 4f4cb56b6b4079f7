#!/usr/bin/env python3
"""Group scorers on one MI355X: what ranking groups by the SUM of their best rows costs.

The corpus, groupings and batches of scripts/probe/grouped_search.py: 40 474 x 768 random unit rows, queries = noisy copies of
rows, device in / device out, hipEvents around the call, median (min .. max) of 25 steps after 5 warm-up steps; `parent_code`-like
(9 726 groups, one of 5 031 rows), `category`-like (2 000 groups of ~20 rows), `level`-like (3 groups of 23 337 / 12 106 / 5 031 rows:
long-group items only). Per (queries, grouping, group_size) at k = 10, the three calls alternating inside every step:
  (a) search_grouped as it always was (icd_index_search_grouped): the baseline;
  (b) scorer="max" through icd_index_search_grouped_scored, no group outputs: the same launches;
  (c) scorer="sum", group outputs on.
`--stages`: one SUM search and one plain grouped search of 10 000 queries per grouping and group_size and nothing else, for
`rocprofv3 --kernel-trace --stats -- python ...`.
Prints a report; `> profiles/group_scorer_probe.log`.
"""
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from grouped_search import DIM, K, N, groupings  # noqa: E402

SIZES = (3, 8)


def main():
    import torch
    from rag_project_icd10_amd._native import IcdIndex
    stages = "--stages" in sys.argv
    rng = np.random.default_rng(77)
    corpus = rng.standard_normal((N, DIM), dtype=np.float32)
    corpus /= np.linalg.norm(corpus, axis=1, keepdims=True)
    qb = np.ascontiguousarray(corpus[rng.integers(0, N, 10000)] + 0.1 * rng.standard_normal((10000, DIM), dtype=np.float32), np.float32)
    index = IcdIndex(corpus, rng.integers(1, 4, N).astype(np.int32), max_nq=10000, max_k=128)
    dq = torch.from_numpy(qb).cuda()
    print(f"corpus: {N} x {DIM} random unit rows; device {torch.cuda.get_device_name(0)}; k = {K}")
    made = {}
    for name, g in groupings(rng).items():
        grouping = index.grouping(g)
        before = grouping.stats()["bytes"]
        grouping.prepare_scorers(index)
        st = grouping.stats()
        made[name] = grouping
        print(f"grouping {name}: {st['groups']} groups, largest {st['largest_group']} rows, the plan and staging add {(st['bytes'] - before) / 2**20:.2f} MiB")
    if stages:
        for name, grouping in made.items():
            for s in SIZES:
                index.search_grouped(dq, K, s, grouping, scorer="sum", group_scores=True)
                index.search_grouped(dq, K, s, grouping)
        torch.cuda.synchronize()
        return

    def timed(calls, steps=25, warm=5):
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

    print("\nnq      grouping           s   (a) grouped ms (min .. max)     (b) scored MAX ms (min .. max)    (c) SUM ms (min .. max)        (c)/(a)")
    for nq in (10000, 1000, 16, 1):
        q = dq[:nq]
        for name, grouping in made.items():
            for s in SIZES:
                (a, alo, ahi), (b, blo, bhi), (c, clo, chi) = timed([
                    lambda: index.search_grouped(q, K, s, grouping),
                    lambda: index.search_grouped(q, K, s, grouping, scorer="max"),
                    lambda: index.search_grouped(q, K, s, grouping, scorer="sum", group_scores=True)])
                print(f"{nq:<7d} {name:<18s} {s:<3d} {a:>8.3f} ({alo:.3f} .. {ahi:.3f})      {b:>8.3f} ({blo:.3f} .. {bhi:.3f})      "
                      f"{c:>8.3f} ({clo:.3f} .. {chi:.3f})    {c / a:>6.2f}")


if __name__ == "__main__":
    main()
