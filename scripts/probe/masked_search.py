#!/usr/bin/env python3
"""Masked search on one MI355X: what a per-query row mask costs next to the plain exact search and next to views
(DESIGN.md section 12).

40 474 x 768 random unit rows (the size of the real ICD-10 corpus), queries = noisy copies of rows, device in / device out,
hipEvents around the call, median of 25 steps after 5 warm-up steps, k = 10. In the SAME run:
  (b) the yardstick, existing code: search_reweighted(mode=MODE_EXACT) at 1 / 16 / 1 000 / 10 000 queries - the same fp32
      products and fused select without a mask;
  (a) search_masked at the same sizes, with ONE mask shared by every query and with 22 distinct masks dealt round-robin, at
      selectivities 0.004 / 0.05 / 0.9 (scattered rows);
  (v) section 9's figures for the same selections: the build of a view, and a search of the CACHED view (its default path) at the
      same sizes - the crossover batch size above which one expression is cheaper as a cached view follows from (a) and (v);
  (c) what a tree without masks must do for the 22-filter batch: 22 view builds + 22 searches (each filter's share of the
      batch), views kept in an LRU of 8 like MilvusService's cache - wall clock, synchronised.
Writes the report to --out (default profiles/masked_search_probe.log) and prints it.
"""
import argparse
import os
import statistics
import sys
import time
from collections import OrderedDict

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

N, DIM, K = 40474, 768, 10
SIZES = (1, 16, 1000, 10000)
SELECTIVITIES = (0.004, 0.05, 0.9)
NMASKS = 22


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "masked_search_probe.log"))
    args = ap.parse_args()
    import torch
    from rag_project_icd10_amd._native import MODE_EXACT, IcdIndex
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    rng = np.random.default_rng(77)
    corpus = rng.standard_normal((N, DIM), dtype=np.float32)
    corpus /= np.linalg.norm(corpus, axis=1, keepdims=True)
    qb = np.ascontiguousarray(corpus[rng.integers(0, N, 10000)] + 0.1 * rng.standard_normal((10000, DIM), dtype=np.float32), np.float32)
    index = IcdIndex(corpus, rng.integers(1, 4, N).astype(np.int32), max_nq=10000, max_k=128)
    dq = torch.from_numpy(qb).cuda()
    say(f"corpus: {N} x {DIM} random unit rows; device {torch.cuda.get_device_name(0)}; k = {K}; median of 25 after 5 warm-up, hipEvents, device in / out")

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

    def selections(sel):
        """NMASKS distinct scattered selections of about sel * N rows each"""
        return [np.sort(np.random.default_rng(1000 + m).choice(N, max(1, int(round(sel * N))), replace=False)).astype(np.int64) for m in range(NMASKS)]

    base = {nq: timed(lambda: index.search_reweighted(dq[:nq], K, MODE_EXACT)) for nq in SIZES}
    say("\n(b) search_reweighted(MODE_EXACT), ms: " + "   ".join(f"nq={nq}: {base[nq]:.4f}" for nq in SIZES))
    say("\n(a) search_masked, ms and ratio to (b)")
    say("selectivity  masks     " + "   ".join(f"nq={nq:<6d}      " for nq in SIZES))
    masked = {}
    for sel in SELECTIVITIES:
        rows = selections(sel)
        masks = [index.rowmask(r) for r in rows]
        for label, pick in (("1 shared", lambda nq: masks[0]), ("22 distinct", lambda nq: [masks[i % NMASKS] for i in range(nq)])):
            cells = []
            for nq in SIZES:
                mk = pick(nq)
                t = timed(lambda: index.search_masked(dq[:nq], K, mk))
                masked[(sel, label, nq)] = t
                cells.append(f"{t:8.4f} ({t / base[nq]:5.2f})")
            say(f"{sel:<11g}  {label:<11s}" + "   ".join(cells))
        st = masks[0].stats()
        say(f"             (a mask: {st['rows']} rows, {st['bytes']} bytes)")
        for m in masks:
            m.close()

    say("\n(v) views of the same selections (section 9's figures in this run): build ms (wall clock, synchronised, median of 5), HBM bytes, "
        "and a search of the CACHED view (search_reweighted, its default path), ms")
    crossover = {}
    for sel in SELECTIVITIES:
        rows = selections(sel)[0]
        builds = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            v = index.view(rows)
            torch.cuda.synchronize()
            builds.append((time.perf_counter() - t0) * 1e3)
            v.close()
        view = index.view(rows)
        st = view.stats()
        hbm = int(st["bytes_corpus_f32"] + st["bytes_corpus_f16"] + st["bytes_workspace"])
        cells = []
        for nq in SIZES:
            t = timed(lambda: view.search_reweighted(dq[:nq], K))
            cells.append(f"nq={nq}: {t:.4f}")
            crossover[(sel, nq)] = (masked[(sel, "1 shared", nq)], t)
        say(f"{sel:<11g}  build {statistics.median(builds):.3f} ms, {hbm / 1e6:.0f} MB;  cached view: " + "   ".join(cells))
        view.close()
    say("\ncrossover, one expression: mask (a, 1 shared) against the CACHED view (v), ms - the smallest measured batch at which the view wins")
    for sel in SELECTIVITIES:
        wins = [nq for nq in SIZES if crossover[(sel, nq)][1] < crossover[(sel, nq)][0]]
        say(f"{sel:<11g}  " + "   ".join(f"nq={nq}: mask {crossover[(sel, nq)][0]:.4f} / view {crossover[(sel, nq)][1]:.4f}" for nq in SIZES) +
            f"   -> view cheaper from nq = {wins[0] if wins else 'never (of the sizes measured)'}")

    say("\n(c) the 22-filter batch without masks: 22 view builds + 22 searches of each filter's share, LRU of 8 views; wall clock ms, synchronised, "
        "median of 3 (every round starts with an empty cache: 22 distinct filters thrash a cache of 8 anyway)")
    for sel in SELECTIVITIES:
        rows = selections(sel)
        for nq in SIZES:
            if nq < NMASKS:
                continue
            share = [torch.arange(m, nq, NMASKS, device=dq.device) for m in range(NMASKS)]
            qs = [dq[:nq][s].contiguous() for s in share]
            ts = []
            for _ in range(3):
                cache = OrderedDict()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for m in range(NMASKS):
                    cache[m] = index.view(rows[m], max_nq=max(16, len(share[m])), max_k=K)
                    cache[m].search_reweighted(qs[m], K)
                    while len(cache) > 8:
                        cache.popitem(last=False)[1].close()
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
                for v in cache.values():
                    v.close()
            a = masked[(sel, "22 distinct", nq)]
            say(f"{sel:<11g}  nq={nq:<6d} views {statistics.median(ts):9.3f} ms   masks (a) {a:8.4f} ms   ratio {statistics.median(ts) / a:7.1f}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
