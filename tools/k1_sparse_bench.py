#!/usr/bin/env python3
"""K1 on sparse features against the dense kernels on the densified matrix, one MI355X, one process.

For an ACM-like shape (N = 3025, F = 1870) and a large one (N = 262 144, F = 2048) at 0.5 %, 2 % and 10 % stored
entries (binary bag-of-words rows with Zipf columns, synth.bag_of_words), times

  * the eval forward             ops.project_fwd(X, ...)                      no dropout
  * the training forward         ops.project_fwd(X, ..., 0.6, 0.6, want_keep=True)
  * dW                           ops.project_bwd(X, dH, ..., 0.6, keep=<the forward's table, if it wrote one>)

with X the SparseFeatures and with X its dense image -- the dense calls are the ones the model makes, keep table
included.  Sparse and dense windows alternate; a window is `inner` back-to-back calls between two HIP events (the
ACM-like calls take tens of microseconds: one call per window would time the events), `reps` windows per side after
a warm-up; median, minimum and maximum per call are reported.  The transposed image of the sparse matrix is built
before the timed windows (it is built once per matrix).  Each line also carries the largest difference between the
two paths' H and dW, the bytes the sparse kernels request per stored entry, and the rate that amounts to.

    python tools/k1_sparse_bench.py [--out profiles/r12_k1_sparse_bench.jsonl] [--reps 20] [--shapes acm,large]
                                     [--densities 0.005,0.02,0.1]

Counters (a run of its own per counter set, few windows): tools/pmc_k1_sparse.sh.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from han_amd import ops, synth  # noqa: E402

SHAPES = {"acm": (3025, 1870, 20), "large": (262144, 2048, 1)}      # N, F, calls per timed window
DENSITIES = (0.005, 0.02, 0.10)
DROP = 0.6


def bag_at_density(n, f, density, seed, dev):
    """A bag-of-words whose stored density is close to `density`: repeated draws of a row count once, so the draws per
    row are raised on a 4096-row sample until the sample is dense enough."""
    want = density * f
    k = max(1, round(want))
    while True:
        s = synth.bag_of_words(n, f, k, seed, device=dev, rows=(0, min(n, 4096)), zipf=0.5)
        got = s.nnz / s.shape[0]
        if got >= 0.97 * want or k >= 8 * f:
            break
        k = max(k + 1, int(k * min(2.0, 1.05 * want / got)))
    return synth.bag_of_words(n, f, k, seed, device=dev, zipf=0.5), k


def timed(sides, reps, inner):
    """sides: {name: fn}; alternating windows of `inner` calls; per-call microseconds (median, min, max) per side."""
    for fn in sides.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in sides}
    for _ in range(reps):
        for k, fn in sides.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            e1.synchronize()
            ts[k].append(e0.elapsed_time(e1) * 1e3 / inner)
    return {k: dict(median=round(sorted(v)[len(v) // 2], 2), min=round(min(v), 2), max=round(max(v), 2))
            for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "r12_k1_sparse_bench.jsonl"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shapes", default="acm,large")
    ap.add_argument("--densities", default=",".join(str(d) for d in DENSITIES))
    ap.add_argument("--chunks", default="128,256,512,1024",
                    help="also time the sparse dW with ops.SPARSE_COL_CHUNK set to each of these ('' = no sweep)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("k1_sparse_bench needs a GPU: a CPU run gives no timing")
    dev = torch.device("cuda:0")
    K, FP, seed = 8, 8, 0x5EED
    g = torch.Generator().manual_seed(1)
    lines = []
    for shape in args.shapes.split(","):
        n, f, inner = SHAPES[shape]
        W = (torch.randn(f, ops.D, generator=g) * 0.1).to(dev)
        a1, a2 = torch.randn(K, FP, generator=g).to(dev), torch.randn(K, FP, generator=g).to(dev)
        b1, b2 = torch.randn(K, generator=g).to(dev), torch.randn(K, generator=g).to(dev)
        dH = torch.randn(n, ops.D, generator=g).to(dev)
        for density in (float(d) for d in args.densities.split(",")):
            xs, draws = bag_at_density(n, f, density, 3, dev)
            xd = xs.to_dense()
            xs.transposed()
            fwd = lambda x, drop, keep=False: ops.project_fwd(x, W, a1, a2, b1, b2, in_drop=drop, fts_drop=drop,
                                                              seed=seed, want_keep=keep)
            # results first: the two paths compute the same numbers (the same draws, another order of the sums)
            Hs, Hd = fwd(xs, 0.0)[0], fwd(xd, 0.0)[0]
            Ts, Td = fwd(xs, DROP, True), fwd(xd, DROP, True)
            keep_d = Td[3]
            bwd = lambda x, keep=None: ops.project_bwd(x, dH, K, FP, in_drop=DROP, seed=seed, keep=keep)
            dWs, dWd = bwd(xs), bwd(xd, keep_d)
            diff = dict(H_eval=float((Hs - Hd).abs().max()), H_train=float((Ts[0] - Td[0]).abs().max()),
                        keep_bits_equal=bool(torch.equal(Ts[0].view(torch.int32) & 1, Td[0].view(torch.int32) & 1)),
                        dW_rel=float((dWs - dWd).abs().max() / dWd.abs().max()))
            t = {}
            t.update({"fwd_eval_" + k: v for k, v in timed({"sparse": lambda: fwd(xs, 0.0), "dense": lambda: fwd(xd, 0.0)},
                                                           args.reps, inner).items()})
            t.update({"fwd_train_" + k: v for k, v in timed({"sparse": lambda: fwd(xs, DROP, True),
                                                             "dense": lambda: fwd(xd, DROP, True)}, args.reps, inner).items()})
            t.update({"dw_" + k: v for k, v in timed({"sparse": lambda: bwd(xs), "dense": lambda: bwd(xd, keep_d)},
                                                     args.reps, inner).items()})
            pair = {s: round(t["fwd_train_" + s]["median"] + t["dw_" + s]["median"], 2) for s in ("sparse", "dense")}
            by_chunk, default_chunk = {}, ops.SPARSE_COL_CHUNK
            for c in (int(v) for v in args.chunks.split(",") if v):      # the chunk table is rebuilt per length (untimed)
                ops.SPARSE_COL_CHUNK = c
                xs.transposed()
                same = bool(torch.allclose(bwd(xs), dWs, rtol=1e-4, atol=1e-4 * float(dWs.abs().max())))
                by_chunk[c] = dict(timed({"sparse": lambda: bwd(xs)}, args.reps, inner)["sparse"],
                                   chunks=xs.transposed()["n_chunks"], same=same)
            ops.SPARSE_COL_CHUNK = default_chunk
            # requested bytes per stored entry: 4 B index + one 256-B row of W (forward) or dH (dW); binary: no value
            req = 4 + 256
            tt = xs.transposed()
            line = dict(tool="k1_sparse_bench", shape=shape, N=n, F=f, density_target=density,
                        density=round(xs.nnz / (n * f), 5), nnz=xs.nnz, draws_per_row=draws, binary=xs.values is None,
                        long_columns=tt["n_long"], chunks=tt["n_chunks"], col_chunk=tt["col_chunk"],
                        dense_keep_table=keep_d is not None, calls_per_window=inner, windows=args.reps, us_per_call=t,
                        dw_sparse_by_chunk=by_chunk, train_pair_us=pair, train_pair_speedup=round(pair["dense"] / pair["sparse"], 3),
                        eval_speedup=round(t["fwd_eval_dense"]["median"] / t["fwd_eval_sparse"]["median"], 3),
                        requested_bytes_per_entry=req,
                        requested_GBps={k: round(xs.nnz * req / (t[k + "_sparse"]["median"] * 1e-6) / 1e9, 1)
                                        for k in ("fwd_eval", "fwd_train", "dw")},
                        max_diff=diff, device=torch.cuda.get_device_name(0))
            print(json.dumps(line), flush=True)
            lines.append(line)
            del xs, xd, Hs, Hd, Ts, Td, dWs, dWd, keep_d
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        for line in lines:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
