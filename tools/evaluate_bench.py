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

--silhouette measures evaluate.silhouette_score (han_silhouette) instead.  The process that is started does not touch
the GPU: it runs one child process per case, each under `timeout` (a case that fails or runs out of time ends the
run), with at most 16 host threads, and appends one JSON line per case to profiles/r14_silhouette_bench.jsonl (or
--out).  Cases: --sil-sklearn (default 20000) rows x 64, k = 4, the device against
sklearn.metrics.silhouette_score on the same host; --sil-device (default 262144) rows, the device alone.  Per case:
  gpu_ms / pairs_per_s   ops.silhouette on rows already grouped (all launches of the call), pairs = N^2 distances;
  score_ms               the whole evaluate.silhouette_score: label codes, sort, gather, the kernels, one read;
  knn_ms / knn_pairs_per_s  ops.knn_topk(x, x, 5) on the same rows in the same run: the same N^2 pair products on the
                         same pipe -- the yardstick of the pair rate;  vs_knn = pairs_per_s / knn_pairs_per_s;
  sklearn_s, score_diff, speedup_vs_sklearn   the sklearn case only (one host run; speed-up of the whole score call).

--tsne measures evaluate.tsne (han_tsne_calibrate / han_tsne_step) and writes profiles/r15_tsne_bench.jsonl (or --out).
ONE child process under `timeout` runs every size of --tsne-sizes (default 3025,4057,20000; perplexity 30), so all the
rates of the file come from one process.  Per size:
  calibrate_ms / passes  the whole ops.tsne_calibrate (row minima, the bisection passes, the reads between batches);
  step_ms, step_kl_ms    one ops.tsne_step without / with the KL sums (median of --reps runs of 20 steps each);
  pairs_per_s            N^2 / step_ms;  sil_pairs_per_s: ops.silhouette on the same rows in the same process, the same
                         N^2 pair products;  vs_silhouette their ratio;
  step_ms_by_width       the step on x repeated to 128, 256 and 512 columns: the tile kernel stages and multiplies one
                         64-column chunk after another (a narrower x is zero-padded to a whole chunk in LDS and costs
                         the same LDS fills and MFMAs, so timing a narrow x isolates nothing), and each further chunk
                         adds one X-tile product -- the LDS fill of both operands and 16 MFMAs per 16 x 16 sub-tile --
                         and nothing of the epilogue;
  chunk_ms               the least-squares slope of step time over chunks (1, 2, 4, 8): what an X-tile product costs
                         where it is NOT hidden.  It is no share of the 64-column step: with one chunk the row tile is
                         staged once per workgroup, with more it is staged again for every column tile, and co-resident
                         workgroups overlap one's product with another's epilogue;
  full_s, n_iter, kl     the whole evaluate.tsne call from a random start (host clock, synchronised);
  sklearn_bh_s           N <= --tsne-bh-max: TSNE(method="barnes_hut"), the host's practical choice, one run.
And records of stage "tsne_exact": per size of --tsne-exact (default 1000,2000,3025: up to where scikit-learn's exact
method ends in about a minute), the device's full call against TSNE(method="exact") on the same host.
"""
import argparse
import json
import os
import subprocess
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


SIL_OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r14_silhouette_bench.jsonl")
HOST_THREADS = 16


def silhouette_case(n, with_sklearn, reps):
    """One case, in a process of its own; returns the record."""
    torch.set_num_threads(min(HOST_THREADS, torch.get_num_threads()))
    dev = torch.device("cuda:0")
    x, y = embeddings(n)
    xt, yt = torch.as_tensor(x).to(dev), torch.as_tensor(y).to(dev)
    order = torch.sort(yt.long(), stable=True).indices
    seg = torch.zeros(5, dtype=torch.int64, device=dev)
    seg[1:] = torch.cumsum(torch.bincount(yt.long(), minlength=4), 0)
    xg = xt[order].contiguous()
    res, ts = gpu_time(lambda: ops.silhouette(xg, seg), reps)
    d = rates(dict(n=n, d=D, stage="silhouette", k=4), n * n, ts)
    score, ts = gpu_time(lambda: evaluate.silhouette_score(xt, yt), reps)
    d.update(score=score, score_ms=round(float(np.median(ts)), 4))
    assert abs(score - float(res["sum"].cpu()[0]) / n) < 1e-12
    _, ts = gpu_time(lambda: ops.knn_topk(xt, xt, 5), reps)
    knn = rates({}, n * n, ts)
    d.update(knn_ms=knn["gpu_ms"], knn_pairs_per_s=knn["pairs_per_s"],
             vs_knn=round(d["pairs_per_s"] / knn["pairs_per_s"], 4))
    if with_sklearn:
        from sklearn.metrics import silhouette_score
        t0 = time.perf_counter()
        ref = float(silhouette_score(x, y, metric="euclidean"))
        d["sklearn_s"] = round(time.perf_counter() - t0, 4)
        d["host_threads"] = int(os.environ.get("OMP_NUM_THREADS", HOST_THREADS))
        d["score_diff"] = abs(ref - score)
        d["speedup_vs_sklearn"] = round(d["sklearn_s"] * 1e3 / d["score_ms"], 1)
    return d


def silhouette_driver(args):
    """One child per case under `timeout`; nothing more is started after a case that fails."""
    env = dict(os.environ)
    for var in ("OMP_NUM_THREADS", "MKL_NUM_THREADS", "OPENBLAS_NUM_THREADS"):
        env[var] = str(min(HOST_THREADS, int(env.get(var) or HOST_THREADS)))
    path = args.out or SIL_OUT
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as out:
        for n, sk in ((args.sil_sklearn, 1), (args.sil_device, 0)):
            if n <= 0:
                continue
            cmd = ["timeout", "-k", "10", str(args.sil_timeout), sys.executable, os.path.abspath(__file__),
                   "--silhouette-case", f"{n},{sk}", "--reps", str(args.reps)]
            r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
            if r.returncode != 0:
                raise SystemExit(f"silhouette case n={n} ended with status {r.returncode}; stopping")
            line = r.stdout.strip().splitlines()[-1]
            print(line, flush=True)
            out.write(line + "\n")
            out.flush()


TSNE_OUT = os.path.join(os.path.dirname(SIL_OUT), "r15_tsne_bench.jsonl")


def _steps_ms(xt, calib, want_kl, reps, steps=20):
    """median ms of one ops.tsne_step over `reps` runs of `steps` steps from the same start"""
    y0 = torch.as_tensor(np.float32(1e-4) * np.random.RandomState(1).standard_normal((xt.shape[0], 2)).astype(np.float32)).to(xt.device)
    lr = max(xt.shape[0] / 48.0, 50.0)

    def run():
        y, u, g = y0.clone(), torch.zeros_like(y0), torch.ones_like(y0)
        for _ in range(steps):
            ops.tsne_step(xt, calib, y, u, g, 12.0, 0.5, lr, want_kl=want_kl)
    return round(float(np.median(gpu_time(run, reps)[1])) / steps, 4)


def _wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def tsne_cases(sizes, exact_sizes, bh_max, reps):
    """Every t-SNE record, in this one process."""
    from sklearn.manifold import TSNE
    torch.set_num_threads(min(HOST_THREADS, torch.get_num_threads()))
    dev = torch.device("cuda:0")
    for n in sizes:
        x, y = embeddings(n)
        xt, yt = torch.as_tensor(x).to(dev), torch.as_tensor(y).to(dev)
        ops.tsne_calibrate(xt, 30.0)                          # warm-up
        calib, t = min((_wall(lambda: ops.tsne_calibrate(xt, 30.0)) for _ in range(reps)), key=lambda r: r[1])
        d = dict(n=n, d=D, stage="tsne", perplexity=30.0, calibrate_ms=round(t * 1e3, 3), passes=int(calib["passes"]),
                 open_rows=int(calib["open_rows"].cpu()[0]))
        d["step_ms"], d["step_kl_ms"] = _steps_ms(xt, calib, False, reps), _steps_ms(xt, calib, True, reps)
        d["pairs_per_s"] = float("%.4g" % (n * n / (d["step_ms"] * 1e-3)))
        by_width = {D: d["step_ms"]}
        for k in (2, 4, 8):
            xw = torch.cat([xt] * k, 1).contiguous()
            by_width[k * D] = _steps_ms(xw, ops.tsne_calibrate(xw, 30.0), False, reps)
            del xw
        d["step_ms_by_width"] = {str(w): t for w, t in by_width.items()}
        d["chunk_ms"] = round(float(np.polyfit([w // D for w in by_width], list(by_width.values()), 1)[0]), 4)
        order = torch.sort(yt.long(), stable=True).indices
        seg = torch.zeros(5, dtype=torch.int64, device=dev)
        seg[1:] = torch.cumsum(torch.bincount(yt.long(), minlength=4), 0)
        xg = xt[order].contiguous()
        sil = rates({}, n * n, gpu_time(lambda: ops.silhouette(xg, seg), reps)[1])
        d.update(sil_ms=sil["gpu_ms"], sil_pairs_per_s=sil["pairs_per_s"],
                 vs_silhouette=round(d["pairs_per_s"] / sil["pairs_per_s"], 4))
        (_, info), t = _wall(lambda: evaluate.tsne(xt, init="random", seed=0, device=dev, return_info=True))
        d.update(full_s=round(t, 4), n_iter=info["n_iter"], kl=round(info["kl_divergence"], 6))
        if n <= bh_max:
            t0 = time.perf_counter()
            TSNE(n_components=2, method="barnes_hut", init="random", random_state=0).fit_transform(x)
            d["sklearn_bh_s"] = round(time.perf_counter() - t0, 3)
            d["host_threads"] = int(os.environ.get("OMP_NUM_THREADS", HOST_THREADS))
        print(json.dumps(d), flush=True)
    for exact_n in exact_sizes:
        x, _ = embeddings(exact_n)
        xt = torch.as_tensor(x).to(dev)
        (_, info), t = _wall(lambda: evaluate.tsne(xt, init="random", seed=0, device=dev, return_info=True))
        t0 = time.perf_counter()
        est = TSNE(n_components=2, method="exact", init="random", random_state=0)
        est.fit_transform(x)
        host = time.perf_counter() - t0
        print(json.dumps(dict(n=exact_n, d=D, stage="tsne_exact", full_s=round(t, 4), n_iter=info["n_iter"],
                              kl=round(info["kl_divergence"], 6), sklearn_exact_s=round(host, 3),
                              sklearn_kl=round(float(est.kl_divergence_), 6), sklearn_n_iter=int(est.n_iter_),
                              host_threads=int(os.environ.get("OMP_NUM_THREADS", HOST_THREADS)),
                              speedup_vs_sklearn=round(host / t, 1))), flush=True)


def tsne_driver(args):
    """One child under `timeout` for all sizes; its lines are the file."""
    env = dict(os.environ)
    for var in ("OMP_NUM_THREADS", "MKL_NUM_THREADS", "OPENBLAS_NUM_THREADS"):
        env[var] = str(min(HOST_THREADS, int(env.get(var) or HOST_THREADS)))
    path = args.out or TSNE_OUT
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    cmd = ["timeout", "-k", "10", str(args.tsne_timeout), sys.executable, os.path.abspath(__file__), "--tsne-case",
           f"{args.tsne_sizes};{args.tsne_exact};{args.tsne_bh_max}", "--reps", str(args.reps)]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    print("\n".join(lines), flush=True)
    if r.returncode != 0:
        raise SystemExit(f"the t-SNE cases ended with status {r.returncode}; nothing written")
    with open(path, "w") as out:
        out.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tsne", action="store_true", help="measure evaluate.tsne (one child for all sizes)")
    ap.add_argument("--tsne-sizes", default="3025,4057,20000")
    ap.add_argument("--tsne-exact", default="1000,2000,3025", help="sizes also run through scikit-learn exact ('': none)")
    ap.add_argument("--tsne-bh-max", type=int, default=4057, help="largest size also run through scikit-learn Barnes-Hut")
    ap.add_argument("--tsne-timeout", type=int, default=540, help="seconds for the t-SNE child")
    ap.add_argument("--tsne-case", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--silhouette", action="store_true", help="measure evaluate.silhouette_score (one child per case)")
    ap.add_argument("--sil-sklearn", type=int, default=20000, help="rows of the case run against scikit-learn (0: skip)")
    ap.add_argument("--sil-device", type=int, default=262144, help="rows of the device-only case (0: skip)")
    ap.add_argument("--sil-timeout", type=int, default=300, help="seconds per silhouette case")
    ap.add_argument("--silhouette-case", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--sizes", default="3025,100000,1000000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--sklearn-max", type=int, default=100000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.silhouette:
        return silhouette_driver(args)
    if args.tsne:
        return tsne_driver(args)
    if not torch.cuda.is_available():
        raise SystemExit("evaluate_bench needs a GPU: there is nothing to measure without one")
    if args.silhouette_case:
        n, sk = (int(v) for v in args.silhouette_case.split(","))
        print(json.dumps(silhouette_case(n, bool(sk), args.reps)), flush=True)
        return
    if args.tsne_case:
        sizes, exact, bh_max = ([int(v) for v in part.split(",") if v] for part in args.tsne_case.split(";"))
        return tsne_cases(sizes, exact, bh_max[0], args.reps)
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
