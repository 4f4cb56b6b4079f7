#!/usr/bin/env python3
"""Hybrid search on one MI355X: what the device-side fuse costs next to the sub-searches it fuses, and next to fusing on the
host.

40 474 x 768 random unit rows (the size of the real ICD-10 corpus), requests = noisy copies of rows, device in / device out,
hipEvents around the call, median of 25 steps after 5 warm-up steps, k = 10. In the SAME run, for nq in 1 / 16 / 1 000 / 3 000,
R in 2 / 3 / 8 and L in 10 / 128:
  (b) the yardstick, existing code: search (AUTO and EXACT) of the nq * R vectors at k = L;
  (a) search_hybrid with RRF and with the weighted ranker (norm "atan"), ms and ratio to (b) in the same mode (AUTO);
  (c) the same fusion done on the host from (b)'s outputs, timed from the moment the lists are on the device (the sub-search is
      NOT in the figure): the device-to-host copy of the whole batch's lists plus a Python dictionary merge per query (what a
      caller does today) - wall clock; the merge is timed on at most 100 queries and the printed figure is scaled to the batch.
Writes the report to --out (default profiles/hybrid_search_probe.log) and prints it.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

N, DIM, K = 40474, 768, 10
SIZES = (1, 16, 1000, 3000)
RS = (2, 3, 8)
LS = (10, 128)


def host_fuse(scores, ids, nq, R, k, c=60.0):
    """RRF on the host from the sub-lists [nq * R, L]: one dictionary per query"""
    out = []
    for q in range(nq):
        acc = {}
        for r in range(R):
            for j, i in enumerate(ids[q * R + r].tolist()):
                if i >= 0:
                    acc[i] = acc.get(i, 0.0) + 1.0 / (c + j + 1)
        out.append(sorted(acc, key=lambda i: (-acc[i], i))[:k])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hybrid_search_probe.log"))
    args = ap.parse_args()
    import torch
    from rag_project_icd10_amd._native import MODE_AUTO, MODE_EXACT, IcdIndex
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    rng = np.random.default_rng(77)
    corpus = rng.standard_normal((N, DIM), dtype=np.float32)
    corpus /= np.linalg.norm(corpus, axis=1, keepdims=True)
    total_max = max(SIZES) * max(RS)
    base = corpus[rng.integers(0, N, max(SIZES))]
    qb = np.repeat(base[:, None, :], max(RS), axis=1) + 0.1 * rng.standard_normal((max(SIZES), max(RS), DIM), dtype=np.float32)
    index = IcdIndex(corpus, rng.integers(1, 4, N).astype(np.int32), max_nq=total_max, max_k=128)
    fusion = index.fusion(total_max)
    dq = torch.from_numpy(np.ascontiguousarray(qb, np.float32)).cuda()
    say(f"corpus: {N} x {DIM} random unit rows; device {torch.cuda.get_device_name(0)}; k = {K}; median of 25 after 5 warm-up, hipEvents, device in / out")
    say(f"fusion workspace: {fusion.stats()['bytes'] / 2**20:.1f} MiB for {total_max} sub-lists")

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

    say("\n  nq  R    L | (b) AUTO  (b) EXACT | (a) RRF   ratio | (a) weighted atan  ratio | (c) host fuse behind (b), wall ms")
    for nq in SIZES:
        for R in RS:
            for L in LS:
                qs = dq[:nq, :R].contiguous()
                flat = qs.reshape(nq * R, DIM)
                b_auto = timed(lambda: index.search(flat, L, MODE_AUTO))
                b_exact = timed(lambda: index.search(flat, L, MODE_EXACT))
                a_rrf = timed(lambda: index.search_hybrid(qs, [L] * R, K, fusion, ranker="rrf"))
                w = [1.0 / (r + 1) for r in range(R)]
                a_w = timed(lambda: index.search_hybrid(qs, [L] * R, K, fusion, ranker="weighted", weights=w, norm="atan"))
                part = min(nq, 100)
                sc, ids = index.search(flat, L, MODE_AUTO)
                torch.cuda.synchronize()   # (b)'s lists are on the device: from here on it is the host's fusion alone
                t0 = time.perf_counter()
                h_sc, h_ids = sc.cpu().numpy(), ids.cpu().numpy()
                t1 = time.perf_counter()
                host_fuse(h_sc, h_ids, part, R, K)
                t2 = time.perf_counter()
                copy_ms, merge_ms = (t1 - t0) * 1e3, (t2 - t1) * 1e3 * (nq / part)
                note = "" if part == nq else f" (merge timed on {part} queries, scaled x {nq / part:.0f})"
                say(f"{nq:5d} {R:2d} {L:4d} | {b_auto:8.4f} {b_exact:9.4f} | {a_rrf:8.4f} {a_rrf / b_auto:6.2f} | {a_w:8.4f} {a_w / b_auto:16.2f} | "
                    f"{copy_ms + merge_ms:9.3f} = copy {copy_ms:.3f} + merge {merge_ms:.3f}{note}")
    fusion.close()
    index.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
