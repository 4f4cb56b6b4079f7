"""Probe of the search by stored ids, one MI355X, through MilvusService. Corpus: 40 474 x 768 unit rows (the
size of the ICD-10 corpus) in tight families of 1 .. 8 rows, the first two rows of every family of three or more bit-identical (a
repeated title), so a row's own hit is not always rank 0. k = 10. Medians of 15 after 3 warm-up steps, the two routes alternating
inside each step; the ranges inside the run are printed. Arms, wall time of the whole call, host lists in and host arrays out:
  by ids       MilvusService.search_by_ids(ids, 10): the ids go to the device, the rows are gathered there, the exact search runs
               at 11 and the row's own hit is cut out there; knn_graph(10) walks every row in chunks of the workspace
  host route   what a caller has without it: the rows' fp32 values out of the host matrix into search_batch at 11 (the default
               route: the certified fp16 coarse pass with exact rescoring - the same lists), the row's own hit dropped in numpy
The two routes' id lists are compared first and the number of differing rows is printed (0 expected: both are exact).
Usage: python scripts/probe/search_by_ids.py > profiles/search_by_ids_probe.log"""
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

N, DIM, K = 40474, 768, 10
STEPS, WARMUP = 15, 3


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def host_route(ms, corpus, ids):
    """the rows' vectors from the host matrix, search_batch at k + 1, self dropped in numpy (absent: the last entry)"""
    adj, raw, hit, _ = ms.search_batch(corpus[ids], K + 1)
    adj, hit = np.asarray(adj), np.asarray(hit)
    at = np.where((hit == ids[:, None]).any(axis=1), (hit == ids[:, None]).argmax(axis=1), K)
    keep = np.arange(K + 1)[None, :] != at[:, None]
    return hit[keep].reshape(len(ids), K), adj[keep].reshape(len(ids), K)


def show(name, ms_):
    print(f"  {name}: median {np.median(ms_):.3f} ms (min {np.min(ms_):.3f}, max {np.max(ms_):.3f})", flush=True)


def run(name, arms, check):
    a, b = check()
    print(f"{name}: the two routes' id lists differ on {int((a != b).any(axis=1).sum())} of {len(a)} rows")
    times = {k: [] for k in arms}
    for step in range(WARMUP + STEPS):
        for k, fn in arms.items():
            t, _ = wall(fn)
            if step >= WARMUP:
                times[k].append(t)
    for k, t in times.items():
        show(k, t)
    m = [np.median(t) for t in times.values()]
    print(f"  by ids / host route = {m[0] / m[1]:.2f}", flush=True)


def main():
    print(f"device: {torch.cuda.get_device_name(0)}; medians of {STEPS} after {WARMUP} warm-up steps, routes alternating inside each step")
    rng = np.random.default_rng(23)
    fam = np.repeat(np.arange(N), rng.integers(1, 9, N))[:N]
    centre = rng.standard_normal((int(fam.max()) + 1, DIM), dtype=np.float32)
    centre /= np.linalg.norm(centre, axis=1, keepdims=True)
    noise = rng.standard_normal((N, DIM), dtype=np.float32)
    corpus = centre[fam] + np.float32(0.05) * noise / np.linalg.norm(noise, axis=1, keepdims=True)
    corpus /= np.linalg.norm(corpus, axis=1, keepdims=True)
    corpus = np.ascontiguousarray(corpus, np.float32)
    sizes = np.bincount(fam)
    second = (np.cumsum(sizes) - sizes)[sizes >= 3] + 1        # the second row of every family of three or more ...
    corpus[second] = corpus[second - 1]                        # ... is a copy of the first
    os.environ["MILVUS_DB_PATH"] = tempfile.mkdtemp(prefix="by_ids_probe_")
    os.environ["MILVUS_COLLECTION_NAME"] = "by_ids_probe"

    class Emb:
        def encode_query(self, t):
            return np.zeros(DIM, np.float32)

    from rag_project_icd10_amd.services.milvus_service import MilvusService
    ms = MilvusService(Emb())
    levels = rng.integers(1, 4, N)
    recs = [{"code": f"X{i:05d}", "preferred_zh": f"title {int(fam[i])}", "level": int(levels[i]), "parent_code": "", "has_complication": False,
             "main_code": None, "secondary_code": None, "category_path": ""} for i in range(N)]
    assert ms.insert_records(recs, list(corpus)) is True
    index = ms._ready_index()
    print(f"corpus: {N} x {DIM} unit rows in {int(fam.max()) + 1} families of 1 .. 8 rows, {len(second)} rows bit-identical to their predecessor; "
          f"index max_nq {index.max_nq}, max_k {index.max_k}")
    for nq in (1, 40, 1000):
        ids = rng.integers(0, N, nq).astype(np.int64)
        if nq > 1:
            ids[1] = second[0]            # a row whose own hit is rank 1, not 0
        run(f"search_by_ids, {nq} ids, k = {K}",
            {"by ids (search_by_ids)": lambda ids=ids: ms.search_by_ids(ids, K),
             "host route (host rows -> search_batch at k + 1 -> numpy)": lambda ids=ids: host_route(ms, corpus, ids)},
            lambda ids=ids: (np.asarray(ms.search_by_ids(ids, K)[2]), host_route(ms, corpus, ids)[0]))
    every = np.arange(N, dtype=np.int64)
    run(f"knn_graph, all {N} rows, k = {K}",
        {"by ids (knn_graph)": lambda: ms.knn_graph(K),
         "host route (host rows -> search_batch at k + 1 -> numpy)": lambda: host_route(ms, corpus, every)},
        lambda: (ms.knn_graph(K)[0], host_route(ms, corpus, every)[0]))
    print(f"by-rows workspace: {ms._workspaces['byrows'][1].stats()['bytes'] / 2**20:.1f} MiB for {ms._workspaces['byrows'][1].max_nq} ids per call")
    ms.disconnect()


if __name__ == "__main__":
    main()
