"""Probe of the keyword match filters, one MI355X: the 40 474 golden titles through the analyzer, the golden
diagnosis strings (cycled to 1 000) as TEXT_MATCH texts at minimum_should_match = 1. Wall-clock medians of 15 after 3 warm-up
steps, each ended by a device synchronisation (both routes hand finished masks to the host):
  masks, device route   IcdIndex.match_masks over the 1 000 term lists (the analysis of the texts is outside, done once)
  masks, host route     SparseTextIndex.match_rows + IcdIndex.rowmask per query
  search, each route    search_masked of 1 000 queries at k = 10 over masks made that way, masks included, masks released
The two routes' masks are compared word for word first.
Usage: python scripts/probe/text_match_masks.py > profiles/text_match_probe.log"""
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


def median_ms(fn, steps=15, warmup=3):
    out = []
    for i in range(warmup + steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warmup:
            out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out)), float(np.min(out)), float(np.max(out))


def main():
    titles = [r["disease"] for r in csv.DictReader(io.StringIO(lzma.open(os.path.join(GOLDEN, "ICD_10v601.csv.xz")).read().decode("utf-8-sig")))]
    strings = [l.strip() for l in open(os.path.join(GOLDEN, "diagnosis_strings.txt"), encoding="utf-8") if l.strip()]
    strings = (strings * (1000 // len(strings) + 1))[:1000]
    tx = sparse_text.SparseTextIndex(titles)
    rng = np.random.default_rng(0)
    n, nq = len(titles), len(strings)
    index = _native.IcdIndex(rng.standard_normal((n, 32), dtype=np.float32), rng.integers(1, 4, n).astype(np.int32), device=0, max_nq=1024,
                             max_k=128, probe=False)
    sp = index.sparse(tx.row_off, tx.terms, tx.vals, tx.vocab_size, max_nq=1024, max_k=128)
    known = []
    for s in strings:
        ids = tx.match_terms(sorted(set(sparse_text.analyze(s)))[:64])[0]
        known.append(ids)
    q_off, q_terms, _ = sparse_text.csr_from_pairs([(k, k) for k in known])
    mm = np.ones(nq, np.int32)
    vocab = np.array(tx.vocab, dtype=object)
    term_lists = [vocab[k].tolist() for k in known]
    print(f"n={n} nq={nq} {sp.stats()} tile={_native.sparse_tile_rows()} terms per query: mean {np.mean([len(k) for k in known]):.1f} max {max(len(k) for k in known)}")

    def device_masks():
        return index.match_masks(sp, q_off, q_terms, mm)

    def host_masks():
        return [index.rowmask(np.flatnonzero(tx.match_rows(t, 1))) for t in term_lists]

    a, b = device_masks(), host_masks()
    rows = [m.stats()["rows"] for m in a]
    assert all(np.array_equal(x.words(), y.words()) for x, y in zip(a, b)) and rows == [m.rows for m in b]
    print(f"the two routes' masks agree word for word; rows per mask: median {int(np.median(rows))} max {max(rows)} empty {rows.count(0)}")
    for m in a + b:
        m.close()
    queries = torch.from_numpy(rng.standard_normal((nq, 32), dtype=np.float32)).cuda()

    def close_all(ms):
        for m in ms:
            m.close()

    def searched(make):
        ms = make()
        index.search_masked(queries, 10, ms)
        close_all(ms)

    for name, fn in (("masks, device route", lambda: close_all(device_masks())), ("masks, host route", lambda: close_all(host_masks())),
                     ("masked search of 1000, device route", lambda: searched(device_masks)), ("masked search of 1000, host route", lambda: searched(host_masks))):
        med, lo, hi = median_ms(fn)
        print(f"{name}: median {med:.2f} ms (min {lo:.2f}, max {hi:.2f}) for {nq} queries")


if __name__ == "__main__":
    main()
