#!/usr/bin/env python3
"""Evaluation of the embeddings on the GPU (han_amd.evaluate: han_knn_topk / han_knn_vote / han_kmeans_step) against
the scikit-learn path on the same host, in the same process.

Synthetic 64-wide embeddings of four overlapping classes, seeded.  One JSON line per (N, stage):
  stage "knn"     one split of my_KNN: train = the first 0.2 N rows, queries = the other 0.8 N, k = 5 -- knn_topk and
                  knn_vote on device tensors;
  stage "kmeans"  one fit of evaluate.kmeans: k = 4, init = the first four rows, tol = 0, max_iter = --iters (the
                  per-iteration read of the `changed` word is part of the fit and of the time), steps = the
                  han_kmeans_step calls of the fit;
  gpu_ms          HIP events around the call, 2 warm-ups, median of --reps (gpu_ms_all: every rep) -- a whole-call
                  time (all launches of the call), not one kernel's;
  pairs           distance pairs of the call (Nq * Nt, or N * k * steps); pairs_per_s = pairs / gpu time;
  mfma_bound_frac 2 * D flop per pair over the time, against 155 TF (the measured fp32-MFMA rate of the part):
                  the share of the matrix-pipe bound the WHOLE call reaches;
  sklearn_s       N <= --sklearn-max only: KNeighborsClassifier(5).fit(train).predict(queries), or
                  KMeans(4, init=the same rows, n_init=1, max_iter=--iters, tol=0).fit, host clock, one run;
  agree           share of queries whose prediction equals scikit-learn's (knn), or of rows whose label does (kmeans).

    python tools/evaluate_bench.py [--out FILE] [--sizes 3025,100000,1000000]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from han_amd import evaluate, ops  # noqa: E402

MFMA_F32_FLOPS = 155e12
D = 64


def embeddings(n, seed=0, classes=4):
    rs = np.random.RandomState(seed)
    y = rs.randint(0, classes, n)
    centres = 0.5 * rs.standard_normal((classes, D))
    return (centres[y] + rs.standard_normal((n, D))).astype(np.float32), y.astype(np.int32)


def gpu_time(fn, reps):
    ts, out = [], None
    for i in range(2 + reps):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        if i >= 2:
            ts.append(e0.elapsed_time(e1))
    return out, ts


def rates(d, pairs, ts):
    med = float(np.median(ts))
    d.update(gpu_ms=round(med, 4), gpu_ms_all=[round(t, 4) for t in ts], pairs=int(pairs),
             pairs_per_s=float("%.4g" % (pairs / (med * 1e-3))),
             mfma_bound_frac=round(2 * D * pairs / (med * 1e-3) / MFMA_F32_FLOPS, 4))
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="3025,100000,1000000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--sklearn-max", type=int, default=100000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("evaluate_bench needs a GPU: there is nothing to measure without one")
    dev = torch.device("cuda:0")
    out = open(args.out, "w") if args.out else None

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    for n in (int(s) for s in args.sizes.split(",")):
        x, y = embeddings(n)
        xt, yt = torch.as_tensor(x).to(dev), torch.as_tensor(y).to(dev)
        split = int(n * 0.2)

        def knn():
            idx, _ = ops.knn_topk(xt[split:], xt[:split], 5)
            return ops.knn_vote(idx, yt[:split])

        pred, ts = gpu_time(knn, args.reps)
        d = rates(dict(n=n, d=D, stage="knn", k=5, n_train=split, n_query=n - split), (n - split) * split, ts)
        macro, micro = evaluate.f1_scores(yt[split:], pred, 4)
        d.update(f1_macro=round(macro, 6), f1_micro=round(micro, 6))
        if n <= args.sklearn_max:
            from sklearn.neighbors import KNeighborsClassifier
            t0 = time.perf_counter()
            ref = KNeighborsClassifier(n_neighbors=5).fit(x[:split], y[:split]).predict(x[split:])
            d["sklearn_s"] = round(time.perf_counter() - t0, 4)
            d["agree"] = round(float((ref == pred.cpu().numpy()).mean()), 6)
            d["speedup_vs_sklearn"] = round(d["sklearn_s"] * 1e3 / d["gpu_ms"], 1)
        emit(d)

        fit, ts = gpu_time(lambda: evaluate.kmeans(xt, 4, init=xt[:4], tol=0, max_iter=args.iters), args.reps)
        steps = len(fit["inertia_history"])
        d = rates(dict(n=n, d=D, stage="kmeans", k=4, max_iter=args.iters, n_iter=fit["n_iter"], steps=steps),
                  n * 4 * steps, ts)
        d["ms_per_step"] = round(d["gpu_ms"] / steps, 4)
        d["inertia"] = fit["inertia"]
        if n <= args.sklearn_max:
            from sklearn.cluster import KMeans
            t0 = time.perf_counter()
            ref = KMeans(n_clusters=4, init=x[:4], n_init=1, max_iter=args.iters, tol=0).fit(x)
            d["sklearn_s"] = round(time.perf_counter() - t0, 4)
            d["sklearn_n_iter"] = int(ref.n_iter_)
            d["agree"] = round(float((ref.labels_ == fit["labels"].cpu().numpy()).mean()), 6)
            d["speedup_vs_sklearn"] = round(d["sklearn_s"] * 1e3 / d["gpu_ms"], 1)
        emit(d)
        del xt, yt, pred, fit
        torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()
