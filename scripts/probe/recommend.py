"""Probe of the recommend search, one MI355X, through the ctypes layer. Corpus: 40 474 x 768 random unit rows
(section 27.7's). Requests of 3 positive and 2 negative stored examples; for nr in {1, 40, 1 000}, k in {10, 1 000} and every
strategy the WHOLE-CALL wall time (ids in, numpy out, the host part included), median of STEPS after WARMUP warm-up steps, the
routes alternating inside each step:
  (a) recommend  IcdRecommend(index).recommend(positive, negative, strategy, k, reweighted=False)
  (b) host       the route a caller has today: the examples' vectors against the corpus on the device (an fp32 matmul: BLAS sums,
                 not the canonical chain), every score pulled to the host, the fold, the exclusion, numpy.argpartition and a sort
                 of the k best in numpy
The ids of (a) and (b) are compared (BLAS sums differ from the canonical chain in the last bits: a few swaps are expected).
The per-kernel split of (a) is not taken here: it needs a kernel trace in a run of its own.
Usage: python scripts/probe/recommend.py > profiles/recommend_probe.log"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

N, DIM = 40474, 768
STEPS, WARMUP = 15, 3
P, NEG = 3, 2


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    from rag_project_icd10_amd import _native
    rng = np.random.default_rng(0)
    corpus = rng.standard_normal((N, DIM), dtype=np.float32)
    corpus /= np.linalg.norm(corpus, axis=1, keepdims=True)
    index = _native.IcdIndex(corpus, None, device=0, max_nq=1024, max_k=128)
    dcorpus = torch.from_numpy(corpus).cuda()
    ws = _native.IcdRecommend(index, 1000, 5000, 1000)
    print(f"recommend probe: n={N} dim={DIM} examples {P}+{NEG} steps={STEPS} warmup={WARMUP} workspace {ws.stats()}", flush=True)
    print("nr k strategy | (a) recommend ms (min max) | (b) host ms | (b)/(a) | ids differing", flush=True)
    for nr in (1, 40, 1000):
        rows = rng.integers(0, N, (nr, P + NEG))
        pos, neg = [r[:P].tolist() for r in rows], [r[P:].tolist() for r in rows]
        drows = torch.from_numpy(rows.reshape(-1)).cuda()
        for k in (10, 1000):
            for strategy in ("average_vector", "best_score", "sum_scores"):
                def route_a():
                    return ws.recommend(pos, neg, strategy, k, reweighted=False)

                def route_b():
                    ex = dcorpus[drows].reshape(nr, P + NEG, DIM)
                    if strategy == "average_vector":
                        mp, mn = ex[:, :P].mean(1), ex[:, P:].mean(1)
                        c = ((mp + (mp - mn)) @ dcorpus.T).cpu().numpy()
                    else:
                        s = (ex.reshape(-1, DIM) @ dcorpus.T).cpu().numpy().reshape(nr, P + NEG, N)
                        if strategy == "sum_scores":
                            c = s[:, :P].sum(1) - s[:, P:].sum(1)
                        else:
                            bp, bn = s[:, :P].max(1), s[:, P:].max(1)
                            c = np.where(bp > bn, bp, -(bn * bn))
                    np.put_along_axis(c, rows, -np.inf, axis=1)
                    part = np.argpartition(-c, k - 1, axis=1)[:, :k]
                    order = np.argsort(-np.take_along_axis(c, part, axis=1), axis=1, kind="stable")
                    return np.take_along_axis(part, order, axis=1)

                diff = int((route_a()[2] != route_b()).sum())
                ta, tb = [], []
                for step in range(WARMUP + STEPS):
                    a_ms, b_ms = wall(route_a)[0], wall(route_b)[0]
                    if step >= WARMUP:
                        ta.append(a_ms), tb.append(b_ms)
                a, b = np.median(ta), np.median(tb)
                print(f"{nr:5d} {k:5d} {strategy:15s} | {a:9.3f} (min {min(ta):.3f} max {max(ta):.3f}) | {b:9.3f} | {b / a:6.2f} | {diff} of {nr * k}", flush=True)
    ws.close()
    index.close()


if __name__ == "__main__":
    main()
