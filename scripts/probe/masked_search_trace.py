#!/usr/bin/env python3
"""Where a masked search's time goes at 10 000 queries: the plain exact search, the band search and the
masked search (22 masks dealt round-robin, one shared mask), 11 calls each, device in / out, on 40 474 x 768 random unit rows,
k = 10. Prints the wall clock per call; run it under `rocprofv3 --kernel-trace --stats -- python3 scripts/probe/masked_search_trace.py`
(a run of its own) for the kernels' share: exact_topk_kernel<16, 1, 4, 60, 16, 2, 32, BAND, MASK> is the sweep of each form."""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from rag_project_icd10_amd._native import MODE_EXACT, IcdIndex
N, DIM, K, NQ = 40474, 768, 10, 10000
rng = np.random.default_rng(77)
corpus = rng.standard_normal((N, DIM), dtype=np.float32)
corpus /= np.linalg.norm(corpus, axis=1, keepdims=True)
qb = np.ascontiguousarray(corpus[rng.integers(0, N, NQ)] + 0.1 * rng.standard_normal((NQ, DIM), dtype=np.float32), np.float32)
index = IcdIndex(corpus, rng.integers(1, 4, N).astype(np.int32), max_nq=NQ, max_k=128)
dq = torch.from_numpy(qb).cuda()
masks = [index.rowmask(np.sort(np.random.default_rng(1000 + m).choice(N, 2024, replace=False))) for m in range(22)]
per_query = [masks[i % 22] for i in range(NQ)]
ceil = torch.full((NQ,), 10.0, device="cuda")
def wall(f, n=10):
    f(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3
print("wall ms per call, 10 000 queries: exact %.3f  band %.3f  masked(22) %.3f  masked(1 shared) %.3f" % (
    wall(lambda: index.search_reweighted(dq, K, MODE_EXACT)), wall(lambda: index.search_range(dq, K, range_filter=ceil)),
    wall(lambda: index.search_masked(dq, K, per_query)), wall(lambda: index.search_masked(dq, K, masks[0]))))
