"""Probe of the MMR search, one MI355X. Corpus: 40 474 x 768 unit rows (the size of the ICD-10 corpus) in
tight families of 1 .. 8 near-identical rows (a family's rows are its centre plus noise of norm 0.05), 1 000 queries = noisy copies
of rows. Shapes: 1 000 queries per call at (k, fetch_k) = (10, 40) and (10, 128), one query per call at (10, 40); lambda 0.5.
Medians of 15 after 3 warm-up steps, the routes alternating inside each step; the ranges inside the run are printed. Arms:
  device route, device time   search_mmr, device in / device out, between two events; and its two parts alone: the sub-search
                              (search_masked at fetch_k, raw form, device in / out) and, by difference, the select kernel
  device route, wall          search_mmr with host queries and host outputs, ended by its own synchronisation
  host route, wall            what the parent commit offers: search_masked(k = fetch_k) with host outputs, the hits' vectors out
                              of the host matrix, and the same greedy loop in numpy (float32 similarities by matrix product, as
                              LangChain's maximal_marginal_relevance does)
The two routes' id lists are compared first: the host route's float32 matrix products are not the canonical chain, so near-ties
may be picked differently; the number of queries whose lists differ is printed, not asserted.
Usage: python scripts/probe/mmr_select.py > profiles/mmr_select_probe.log"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from rag_project_icd10_amd import _native  # noqa: E402

N, DIM, K, LAM = 40474, 768, 10, 0.5
STEPS, WARMUP = 15, 3


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def device(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def host_route(index, corpus, q, fetch_k):
    """search at fetch_k, the hits' vectors from the host matrix, the greedy loop in numpy"""
    raw, ids, _ = index.search_masked(q, fetch_k, [None] * len(q), reweighted=False)
    out = np.full((len(q), K), -1, np.int64)
    for i in range(len(q)):
        c = int((ids[i] >= 0).sum())
        vec = corpus[ids[i][:c]]
        sim = vec @ vec.T
        rel = raw[i][:c].astype(np.float64)
        picks = [0]
        pen = sim[0].astype(np.float64).copy()
        left = np.ones(c, bool)
        left[0] = False
        while len(picks) < min(K, c):
            val = np.where(left, LAM * rel - (1.0 - LAM) * pen, -np.inf)
            j = int(np.argmax(val))
            picks.append(j)
            left[j] = False
            pen = np.maximum(pen, sim[j])
        out[i, :len(picks)] = ids[i][picks]
    return out


def show(name, ms):
    print(f"  {name}: median {np.median(ms):.3f} ms (min {np.min(ms):.3f}, max {np.max(ms):.3f})", flush=True)


def run(index, mmr, corpus, q, fetch_k):
    nq = len(q)
    qd = torch.from_numpy(q).cuda()
    none = [None] * nq
    got = index.search_mmr(q, K, fetch_k, LAM, mmr=mmr, reweighted=False)[2]
    ref = host_route(index, corpus, q, fetch_k)
    differ = int((got != ref).any(axis=1).sum())
    print(f"nq = {nq}, k = {K}, fetch_k = {fetch_k}, lambda = {LAM}: the two routes' id lists differ on {differ} of {nq} queries")
    arms = {
        "device route, device time (sub-search + select)": lambda: device(lambda: index.search_mmr(qd, K, fetch_k, LAM, mmr=mmr, reweighted=False)),
        "sub-search alone, device time": lambda: device(lambda: index.search_masked(qd, fetch_k, none, reweighted=False)),
        "device route, wall (host in / out)": lambda: wall(lambda: index.search_mmr(q, K, fetch_k, LAM, mmr=mmr, reweighted=False)),
        "host route, wall (search + host vectors + numpy)": lambda: wall(lambda: host_route(index, corpus, q, fetch_k)),
    }
    times = {k: [] for k in arms}
    for step in range(WARMUP + STEPS):
        for k, fn in arms.items():
            ms, _ = fn()
            if step >= WARMUP:
                times[k].append(ms)
    for k, ms in times.items():
        show(k, ms)
    whole, sub = np.median(times["device route, device time (sub-search + select)"]), np.median(times["sub-search alone, device time"])
    print(f"  select kernel by difference: {whole - sub:.3f} ms = {100 * (whole - sub) / whole:.0f} % of the device time; sub-search {100 * sub / whole:.0f} %", flush=True)


def main():
    print(f"device: {torch.cuda.get_device_name(0)}; medians of {STEPS} after {WARMUP} warm-up steps, routes alternating inside each step")
    rng = np.random.default_rng(21)
    fam = np.repeat(np.arange(N), rng.integers(1, 9, N))[:N]
    centre = rng.standard_normal((int(fam.max()) + 1, DIM), dtype=np.float32)
    centre /= np.linalg.norm(centre, axis=1, keepdims=True)
    noise = rng.standard_normal((N, DIM), dtype=np.float32)
    corpus = centre[fam] + np.float32(0.05) * noise / np.linalg.norm(noise, axis=1, keepdims=True)
    corpus /= np.linalg.norm(corpus, axis=1, keepdims=True)
    corpus = np.ascontiguousarray(corpus, np.float32)
    q = corpus[rng.integers(0, N, 1000)] + np.float32(0.02) * rng.standard_normal((1000, DIM), dtype=np.float32)
    q = np.ascontiguousarray(q / np.linalg.norm(q, axis=1, keepdims=True), np.float32)
    index = _native.IcdIndex(corpus, rng.integers(1, 4, N).astype(np.int32), device=0, max_nq=1024, max_k=128)
    mmr = index.mmr()
    print(f"corpus: {N} x {DIM} unit rows in {int(fam.max()) + 1} families of 1 .. 8 near-identical rows; workspace {mmr.stats()['bytes'] / 2**20:.1f} MiB")
    run(index, mmr, corpus, q, 40)
    run(index, mmr, corpus, q, 128)
    run(index, mmr, corpus, q[:1], 40)


if __name__ == "__main__":
    main()
