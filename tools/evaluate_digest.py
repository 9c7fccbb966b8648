#!/usr/bin/env python3
"""sha256 of every output of the evaluation kernels (han_amd/csrc/evaluate.hip) on a fixed case list, through the
public han_amd.ops wrappers: one JSON line per case.  Two trees whose kernels compute the same bits print the same
lines, so a refactor of evaluate.hip is checked by running this file in the parent tree and in the new one (a fresh
process each) and comparing the outputs line for line.

    python tools/evaluate_digest.py [--out FILE]

The inputs are those of the GPU tests, so every kernel path is reached at the smallest shape that reaches it:
  knn        EXACT, REAL and the strided case of tests/test_evaluate_gpu.py (all three list sizes, one and several
             64-column stages, widths that are no multiple of 4, one and several train-set splits, fewer than 64 train
             rows), each with knn_vote on its neighbours and contingency on the votes;
  kmeans     kmeans_step for k in {1, 3, 4, 17, 64} x D in {13, 64}, the integer rows of the test and the same rows
             with noise (so that roundings show), with and without prev;
  silhouette the five CASES of tests/test_silhouette_gpu.py (one split: a and b finished in the tile kernel; slabs);
  tsne       the six CASES of tests/test_tsne_gpu.py: tsne_calibrate at perplexity 10 and 30, then tsne_step from the
             wide and the 1e-4 start with and without want_kl and want_grad.
A digest covers dtype, shape and bytes.  Nothing is compared here and nothing is timed."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from han_amd import ops  # noqa: E402
from tests import silhouette_ref, tsne_ref  # noqa: E402
from tests import test_evaluate_gpu as te  # noqa: E402
from tests import test_silhouette_gpu as ts  # noqa: E402
from tests import test_tsne_gpu as tt  # noqa: E402


def digest(t):
    if t is None:
        return None
    a = np.ascontiguousarray(t.detach().cpu().numpy())
    return hashlib.sha256(f"{a.dtype}{a.shape}".encode() + a.tobytes()).hexdigest()


def knn_cases(dev):
    for nq, nt, d, k, r, dup in te.EXACT:
        rs = np.random.RandomState(nq + nt + d + k + r)
        q, t = te._ints(rs, (nq, d), r), te._ints(rs, (nt, d), r)
        if dup:
            t[nt // 2:nt // 2 + nt // 4] = t[:nt // 4]
        yield f"knn exact {nq}x{nt}x{d} k{k} r{r} dup{int(dup)}", te._t(q, dev), te._t(t, dev), k, rs
    for nq, nt, d, k in te.REAL:
        q, t, _, _ = te._real_case(nq, nt, d, k)
        yield f"knn real {nq}x{nt}x{d} k{k}", te._t(q, dev), te._t(t, dev), k, np.random.RandomState(nq + k)
    rs = np.random.RandomState(3)
    big_q, big_t = te._ints(rs, (40, 24), 8), te._ints(rs, (300, 20), 8)
    yield "knn strided 40x300x13 k4", te._t(big_q, dev)[:, 3:16], te._t(big_t, dev)[:, 5:18], 4, rs


def knn(dev):
    for name, q, t, k, rs in knn_cases(dev):
        labels = te._t(rs.randint(0, 4, t.shape[0]).astype(np.int32), dev)
        truth = te._t(rs.randint(0, 4, q.shape[0]).astype(np.int32), dev)
        idx, d2 = ops.knn_topk(q, t, k)
        pred = ops.knn_vote(idx, labels)
        yield name, dict(idx=idx, d2=d2, pred=pred, table=ops.contingency(truth, pred, 4, 4))


def kmeans(dev):
    for d in (13, 64):
        for k in (1, 3, 4, 17, 64):
            rs = np.random.RandomState(10 * d + k)
            n = 1003
            x, c = te._ints(rs, (n, d), 8), te._ints(rs, (k, d), 8)
            if k >= 3:
                c[1] = c[0]
                c[k - 1] = 100.0
            prev = te._t(rs.randint(0, k, n).astype(np.int32), dev)
            noise = (0.37 * rs.standard_normal((n, d))).astype(np.float32)
            for kind, rows in (("int", x), ("real", x + noise)):
                for with_prev in (True, False):
                    out = ops.kmeans_step(te._t(rows, dev), te._t(c, dev), prev if with_prev else None, want_d2=with_prev)
                    yield f"kmeans {kind} k{k} d{d} prev{int(with_prev)}", out


def silhouette(dev):
    for name, (sizes, dim, spread) in ts.CASES.items():
        x, _, seg = silhouette_ref.blobs(len(name) + dim, sizes, dim, spread)
        yield f"silhouette {name}", ops.silhouette(te._t(x, dev), te._t(seg, dev))


def tsne(dev):
    for name, (n, dim, scale, dup) in tt.CASES.items():
        x = tsne_ref.blobs(n + dim, n, dim, spread=1.5)[0] * np.float32(scale)
        if dup:
            x[[40, 90]] = x[3]
            x[[41, 129]] = x[64]
        xt = te._t(x, dev)
        lr = max(n / 12.0 / 4.0, 50.0)
        for perplexity in (10.0, 30.0):
            calib = ops.tsne_calibrate(xt, perplexity)
            yield f"tsne calibrate {name} p{perplexity:g}", calib
            for kind in ("wide", "init"):
                for want_kl in (True, False):
                    for want_grad in (True, False):
                        y = te._t(tt._start(name, kind), dev)
                        update, gains = torch.zeros_like(y), torch.ones_like(y)
                        r = ops.tsne_step(xt, calib, y, update, gains, 12.0, 0.5, lr, want_grad=want_grad, want_kl=want_kl)
                        yield (f"tsne step {name} p{perplexity:g} {kind} kl{int(want_kl)} grad{int(want_grad)}",
                               dict(y=y, update=update, gains=gains, stats=r["stats"], grad=r["grad"]))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("evaluate_digest needs a GPU: the digests are of what the kernels compute")
    dev = torch.device("cuda:0")
    out = open(args.out, "w") if args.out else None
    for family in (knn, kmeans, silhouette, tsne):
        for name, tensors in family(dev):
            line = json.dumps(dict(case=name, sha256={key: digest(t) for key, t in tensors.items()}))
            print(line, flush=True)
            if out:
                out.write(line + "\n")
    if out:
        out.close()


if __name__ == "__main__":
    main()
