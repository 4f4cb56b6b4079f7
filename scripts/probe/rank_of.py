"""Probe of the rank-of search, one MI355X, through the ctypes layer. Corpus: 40 474 x 768 unit rows (the size of the
ICD-10 corpus) in tight families of 1 .. 8 rows; one gold row per query: for four queries in five the row the query is a noisy
copy of, for the fifth a random row (a labelled pair the pipeline gets wrong: its rank is what an evaluation wants to see).
Medians of 15 after 3 warm-up steps, the three routes alternating inside each step; the ranges inside the run are printed. Wall
time of the whole call around a device synchronisation, host queries in and host arrays out:
  rank_of      IcdRankOf(index).rank_of(queries, gold): the targets' scores, then ONE counting sweep
  (a) search   the exact search at k = 128 (search_range without a bound: icd_index_search_masked's path without a table), the gold
               id looked up in the 128 ids on the host; the share of gold rows it does not find is printed
  (b) scores   every score of every query pulled to the host (an fp32 matmul on the device, one copy) and ranked in numpy
The ranks of rank_of and of (a), where (a) finds the row, are compared first (0 differences expected: both are exact); (b)'s
scores are BLAS sums, not the canonical chain, so its ranks may differ on near-ties and are only counted.
The device span of a rank_of call (two events around it, device queries) is printed next to its wall time.
Usage: python scripts/probe/rank_of.py > profiles/rank_of_probe.log"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

N, DIM, K = 40474, 768, 128
STEPS, WARMUP = 15, 3


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def show(name, ms_):
    print(f"  {name}: median {np.median(ms_):.3f} ms (min {np.min(ms_):.3f}, max {np.max(ms_):.3f})", flush=True)


def main():
    from rag_project_icd10_amd._native import IcdIndex, IcdRankOf
    print(f"device: {torch.cuda.get_device_name(0)}; medians of {STEPS} after {WARMUP} warm-up steps, routes alternating inside each step")
    rng = np.random.default_rng(29)
    fam = np.repeat(np.arange(N), rng.integers(1, 9, N))[:N]
    centre = rng.standard_normal((int(fam.max()) + 1, DIM), dtype=np.float32)
    centre /= np.linalg.norm(centre, axis=1, keepdims=True)
    noise = rng.standard_normal((N, DIM), dtype=np.float32)
    corpus = centre[fam] + np.float32(0.05) * noise / np.linalg.norm(noise, axis=1, keepdims=True)
    corpus /= np.linalg.norm(corpus, axis=1, keepdims=True)
    corpus = np.ascontiguousarray(corpus, np.float32)
    levels = rng.integers(1, 4, N).astype(np.int32)
    index = IcdIndex(corpus, levels, device=0, max_nq=1024, max_k=K, probe=False)
    ws = IcdRankOf(index)
    dcorpus = torch.from_numpy(corpus).cuda()
    print(f"corpus: {N} x {DIM} unit rows in {int(fam.max()) + 1} families of 1 .. 8 rows; rank-of workspace {ws.stats()['bytes'] / 2**20:.1f} MiB for {ws.max_nq} queries")
    for nq in (1, 40, 1000):
        src = rng.integers(0, N, nq)
        qn = rng.standard_normal((nq, DIM), dtype=np.float32)
        q = corpus[src] + np.float32(0.3) * qn / np.linalg.norm(qn, axis=1, keepdims=True)
        q = np.ascontiguousarray(q / np.linalg.norm(q, axis=1, keepdims=True), np.float32)
        gold = src.astype(np.int64)
        wrong = np.arange(nq) % 5 == 4
        gold[wrong] = rng.integers(0, N, int(wrong.sum()))
        gold = gold.reshape(nq, 1)

        def route_rank():
            return ws.rank_of(q, gold)[0][:, 0]

        def route_search():
            _raw, ids, _lv = index.search_range(q, K, reweighted=False)
            hit = ids == gold
            return np.where(hit.any(axis=1), hit.argmax(axis=1), -1)

        def route_scores():
            sc = (torch.from_numpy(q).cuda() @ dcorpus.T).cpu().numpy()
            sg = sc[np.arange(nq), gold[:, 0]][:, None]
            return (sc > sg).sum(axis=1) + ((sc == sg) & (np.arange(N)[None, :] < gold)).sum(axis=1)

        r, a, b = route_rank(), route_search(), route_scores()
        found = a >= 0
        print(f"{nq} queries, one gold row each: (a) finds {int(found.sum())} of {nq} gold rows in its {K} hits ({100.0 * (1 - found.mean()):.1f} % lost; "
              f"largest rank {int(r.max())}); rank_of and (a) differ on {int((r[found] != a[found]).sum())} of the found; rank_of and (b) differ on {int((r != b).sum())} of {nq}")
        arms = {"rank_of": route_rank, "(a) search at k = 128 + host lookup": route_search, "(b) all scores to the host + numpy": route_scores}
        times = {k: [] for k in arms}
        for step in range(WARMUP + STEPS):
            for k, fn in arms.items():
                t, _ = wall(fn)
                if step >= WARMUP:
                    times[k].append(t)
        for k, t in times.items():
            show(k, t)
        m = [np.median(t) for t in times.values()]
        print(f"  rank_of / (a) = {m[0] / m[1]:.2f}; rank_of / (b) = {m[0] / m[2]:.3f}", flush=True)
        dq = torch.from_numpy(q).cuda()
        spans = []
        for step in range(WARMUP + STEPS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            ws.rank_of(dq, gold)
            e1.record()
            torch.cuda.synchronize()
            if step >= WARMUP:
                spans.append(e0.elapsed_time(e1))
        show("rank_of, device queries: span between two events around the call (targets' copy, both kernels, outputs' copies)", spans)
    ws.close()
    index.close()


if __name__ == "__main__":
    main()
