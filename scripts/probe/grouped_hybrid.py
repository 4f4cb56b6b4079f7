"""Grouped sparse and grouped hybrid search against their yardsticks, one run on one MI355X.

40 474 x 768 random unit rows plus the BM25 index of the golden titles, grouped by the three-character category of the code. Device
in / device out, hipEvents, median of 25 after 5 warm-ups. Each configuration is timed next to plain `search_sparse` at k * s in
the same run; `search_hybrid` grouped is timed next to `search_grouped` of its nq * R vectors. Writes
profiles/grouped_hybrid_probe.log.

    python scripts/probe/grouped_hybrid.py
"""
import csv
import io
import lzma
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from rag_project_icd10_amd import _native   # noqa: E402
from rag_project_icd10_amd.services import sparse_text   # noqa: E402

WARM, REPS = 5, 25


def timed(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def main():
    rd = csv.DictReader(io.StringIO(lzma.open(os.path.join(ROOT, "tests", "golden", "ICD_10v601.csv.xz")).read().decode("utf-8-sig")))
    recs = list(rd)
    titles = [r["disease"] for r in recs]
    n = len(titles)
    where = {c: i for i, c in enumerate(sorted({r["code"][:3] for r in recs}))}
    group_of = np.array([where[r["code"][:3]] for r in recs], np.int32)
    rng = np.random.default_rng(0)
    corpus = rng.standard_normal((n, 768), dtype=np.float32)
    corpus /= np.linalg.norm(corpus, axis=1, keepdims=True)
    index = _native.IcdIndex(corpus, rng.integers(1, 4, n).astype(np.int32), device=0, max_nq=3000, max_k=128)
    tx = sparse_text.SparseTextIndex(titles)
    sp = index.sparse(tx.row_off, tx.terms, tx.vals, tx.vocab_size, max_nq=1024, max_k=128)
    grouping = index.grouping(group_of, max_nq=1024)
    lines = [f"n={n} vocab={tx.vocab_size} nnz={sp.stats()['nnz']} groups={grouping.stats()['groups']} largest={grouping.stats()['largest_group']}",
             f"warm-ups {WARM}, median of {REPS}, hipEvents, device in / device out, validate=False",
             "nq    k   s   grouped_ms   plain_at_k*s_ms   ratio"]
    for nq in (1, 16, 1000):
        q = tx.encode_queries([titles[i] for i in rng.integers(0, n, nq)])
        dq = (torch.from_numpy(q[0]).cuda(), torch.from_numpy(q[1].view(np.int32)).cuda(), torch.from_numpy(q[2]).cuda())
        for k, s in ((10, 1), (10, 3)):
            g_ms = timed(lambda: index.search_sparse(sp, *dq, k, reweighted=True, validate=False, grouping=grouping, group_size=s))
            p_ms = timed(lambda: index.search_sparse(sp, *dq, k * s, reweighted=True, validate=False))
            lines.append(f"{nq:<5d} {k:<3d} {s:<3d} {g_ms:10.3f}   {p_ms:15.3f}   {g_ms / p_ms:5.2f}")
    # search_hybrid grouped against search_grouped of the nq * R vectors (its own sub-search alone)
    fusion = index.fusion(3000)
    g_big = index.grouping(group_of, max_nq=3000)
    lines += ["", "nq    R   L    hybrid_grouped_ms   search_grouped_nq*R_ms   ratio"]
    for nq in (16, 1000):
        for R in (2, 3):
            for L in (10, 40):
                src = torch.from_numpy(corpus[rng.integers(0, n, nq * R)] + 0.05 * rng.standard_normal((nq * R, 768), dtype=np.float32)).cuda()
                h_ms = timed(lambda: index.search_hybrid(src.reshape(nq, R, 768), [L] * R, 10, fusion, grouping=g_big, group_size=3))
                y_ms = timed(lambda: index.search_grouped(src, L, 3, g_big))
                lines.append(f"{nq:<5d} {R:<3d} {L:<4d} {h_ms:17.3f}   {y_ms:22.3f}   {h_ms / y_ms:5.2f}")
    lines += ["", "where a ratio exceeds 2 at nq = 1000: split the kernels with a separate `rocprofv3 --kernel-trace --stats -- python scripts/probe/grouped_hybrid.py`"]
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    out = os.path.join(ROOT, "profiles", "grouped_hybrid_probe.log")
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
