#!/usr/bin/env python3
"""Boosted search on one MI355X: what a boost costs next to the masked search it rides on, and what the existing searches cost
in THIS build.

40 474 x 768 random unit rows (the size of the real ICD-10 corpus), queries = noisy copies of rows, device in / device out,
hipEvents around the call, median of 25 steps after 5 warm-up steps, k = 10. In the SAME run:
  (e) existing code, for a comparison of two builds: plain exact (search_reweighted, MODE_EXACT), range (search_range with a floor)
      and masked (search_masked, 22 distinct masks of half the rows) at 1 / 40 / 10 000 queries, each measured `--repeats` times
      so that the spread of one build's own runs is on the page;
  (b) the baseline of a boost: search_masked on the same batch (a filter mask on every query), at 1 / 40 / 1 000 queries;
  (a) search_boosted on that batch with 1 and with 4 boosts per query (distinct masks of a tenth of the rows, dealt round-robin)
      and the ratio to (b), the boosts as a prepared _native.BoostTable (the device's cost) and as per-query Python lists walked on
      every call (what a caller who builds them per call sees); a single query per call from the host as well;
  (h) the host alternative for the 1 000 queries: the raw scores of ALL rows to the host (torch matmul on the device, one copy of
      1 000 x 40 474 floats) + numpy multiply and argpartition - wall clock, synchronised.
Writes the report to --out (default profiles/boosted_search_probe.log) and prints it.
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
NMASKS = 22


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "boosted_search_probe.log"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--existing-only", action="store_true", help="part (e) alone: runs on a build without the boosted search")
    args = ap.parse_args()
    import torch
    from rag_project_icd10_amd import _native
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

    def selection(seed, share):
        return np.sort(np.random.default_rng(seed).choice(N, int(round(share * N)), replace=False)).astype(np.int64)

    filters = [index.rowmask(selection(1000 + m, 0.5)) for m in range(NMASKS)]
    say(f"\n(e) existing searches in this build, ms ({args.repeats} runs each, every run a median of 25)")
    for nq in (1, 40, 10000):
        fm = [filters[i % NMASKS] for i in range(nq)]
        for label, f in (("plain exact", lambda: index.search_reweighted(dq[:nq], K, MODE_EXACT)),
                         ("range", lambda: index.search_range(dq[:nq], K, radius=0.05)),
                         ("masked", lambda: index.search_masked(dq[:nq], K, fm))):
            runs = [timed(f) for _ in range(args.repeats)]
            say(f"nq={nq:<6d} {label:<12s} " + "  ".join(f"{t:8.4f}" for t in runs) + f"   spread {100 * (max(runs) - min(runs)) / min(runs):.1f} %")
    if not args.existing_only:
        ws = index.boost_workspace(10000)
        boosts = [index.rowmask(selection(2000 + m, 0.1)) for m in range(NMASKS)]
        say("\n(b) search_masked and (a) search_boosted on the same batch, ms and ratio to (b)")
        for nq in (1, 40, 1000):
            fm = [filters[i % NMASKS] for i in range(nq)]
            b = timed(lambda: index.search_masked(dq[:nq], K, fm))
            cells = [f"masked {b:8.4f}"]
            for nb in (1, 4):
                lists = [[(boosts[(i + j) % NMASKS], 1.5 - 0.2 * j) for j in range(nb)] for i in range(nq)]
                table = _native.BoostTable(lists, nq)
                t = timed(lambda: index.search_boosted(dq[:nq], K, table, fm, workspace=ws))
                tl = timed(lambda: index.search_boosted(dq[:nq], K, lists, fm, workspace=ws))
                cells.append(f"{nb} boost{'s' if nb > 1 else ' '} {t:8.4f} ({t / b:5.2f}), as lists {tl:8.4f} ({tl / b:5.2f})")
            say(f"nq={nq:<6d} " + "   ".join(cells))
        hq = qb[:1]
        for label, f in (("masked", lambda: index.search_masked(hq, K, [filters[0]])),
                         ("1 boost", lambda: index.search_boosted(hq, K, [[(boosts[0], 1.5)]], [filters[0]], workspace=ws)),
                         ("4 boosts", lambda: index.search_boosted(hq, K, [[(boosts[j], 1.5 - 0.2 * j) for j in range(4)]], [filters[0]], workspace=ws))):
            ts = []
            for i in range(205):
                t0 = time.perf_counter()
                f()
                ts.append((time.perf_counter() - t0) * 1e6)
            say(f"one query per call from the host, {label:<8s}: {statistics.median(ts[5:]):7.1f} us wall clock (median of 200)")
        say("\n(h) the host alternative for 1 000 queries: all raw scores to the host + numpy (multiply, argpartition, sort of the 10), wall clock ms, median of 3")
        dc = torch.from_numpy(corpus).cuda()
        member = np.zeros((NMASKS, N), bool)
        for m in range(NMASKS):
            member[m, selection(2000 + m, 0.1)] = True
        ts = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            scores = (dq[:1000] @ dc.T).cpu().numpy()
            t1 = time.perf_counter()
            for i in range(1000):
                scores[i, member[i % NMASKS]] *= np.float32(1.5)
            top = np.argpartition(-scores, K, axis=1)[:, :K]
            np.take_along_axis(top, np.argsort(-np.take_along_axis(scores, top, 1), axis=1), 1)
            ts.append(((t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3))
        say(f"scores to the host {statistics.median(t[0] for t in ts):8.2f} ms + numpy {statistics.median(t[1] for t in ts):8.2f} ms"
            " (one boost, no filter; the device product is torch's, not the canonical chain)")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
