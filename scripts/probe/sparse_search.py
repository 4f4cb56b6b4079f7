"""Probe of the sparse search, one MI355X: the 40 474 golden titles through the analyzer and BM25, the
golden diagnosis strings as queries, device in / device out, hipEvents, median of 25 after 5 warm-up steps.
  (a) search_sparse at nq 1 / 16 / 1 000, k 10 / 128   (b) the dense EXACT search at the same nq and k
  (c) fuse_lists over dense + sparse against search_hybrid over dense + dense, R = 2   (d) index build time and bytes
Usage: python scripts/probe/sparse_search.py > profiles/sparse_search_probe.log"""
import csv
import io
import lzma
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from rag_project_icd10_amd import _native  # noqa: E402
from rag_project_icd10_amd.services import sparse_text  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def median_ms(fn, steps=25, warmup=5):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def main():
    titles = [r["disease"] for r in csv.DictReader(io.StringIO(lzma.open(os.path.join(GOLDEN, "ICD_10v601.csv.xz")).read().decode("utf-8-sig")))]
    strings = [l.strip() for l in open(os.path.join(GOLDEN, "diagnosis_strings.txt"), encoding="utf-8") if l.strip()]
    strings = (strings * (1000 // len(strings) + 1))[:1000]
    t0 = time.perf_counter()
    tx = sparse_text.SparseTextIndex(titles)
    t_text = time.perf_counter() - t0
    rng = np.random.default_rng(0)
    n, dim = len(titles), 768
    corpus = rng.standard_normal((n, dim), dtype=np.float32)
    corpus /= np.linalg.norm(corpus, axis=1, keepdims=True)
    index = _native.IcdIndex(corpus, rng.integers(1, 4, n).astype(np.int32), device=0, max_nq=2048, max_k=128)
    t0 = time.perf_counter()
    sp = index.sparse(tx.row_off, tx.terms, tx.vals, tx.vocab_size, max_nq=1024, max_k=128)
    print(f"(d) analyzer + BM25 {t_text:.2f} s, pack + upload {time.perf_counter() - t0:.3f} s, {sp.stats()}")
    q_all = tx.encode_queries(strings)
    _native.check_sparse_rows(*q_all, tx.vocab_size, 64, "query")
    dense_q = torch.from_numpy(rng.standard_normal((1000, dim), dtype=np.float32)).cuda()
    dense_q /= dense_q.norm(dim=1, keepdim=True)
    for nq in (1, 16, 1000):
        off = q_all[0][:nq + 1]
        dq = (torch.from_numpy(off.copy()).cuda(), torch.from_numpy(q_all[1][:off[-1]].view(np.int32).copy()).cuda(), torch.from_numpy(q_all[2][:off[-1]].copy()).cuda())
        for k in (10, 128):
            a = median_ms(lambda: index.search_sparse(sp, *dq, k, validate=False))   # (checked once above, on the host: only enqueues)
            b = median_ms(lambda: index.search(dense_q[:nq], k, _native.MODE_EXACT))
            print(f"(a, b) nq={nq} k={k}: search_sparse {a:.3f} ms, dense EXACT {b:.3f} ms")
        if nq * 2 <= index.max_nq:
            fusion = index.fusion(nq * 2)
            two = torch.stack([dense_q[:nq], dense_q[:nq].flip(0)], dim=1).contiguous()

            def dense_sparse():
                d_raw, d_ids = index.search(dense_q[:nq], 10, _native.MODE_EXACT)
                s_raw, s_ids, _ = index.search_sparse(sp, *dq, 10, validate=False)
                return index.fuse_lists(fusion, torch.stack([d_raw, s_raw], dim=1), torch.stack([d_ids, s_ids], dim=1), 10, 10)
            c1 = median_ms(dense_sparse)
            c2 = median_ms(lambda: index.search_hybrid(two, 10, 10, fusion, mode=_native.MODE_EXACT))
            print(f"(c) nq={nq} R=2 k=10: dense + sparse {c1:.3f} ms, dense + dense {c2:.3f} ms")
            fusion.close()
    sp.close()
    index.close()


if __name__ == "__main__":
    main()
