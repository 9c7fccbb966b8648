#!/usr/bin/env python3
"""Meta-path construction on the GPU (han_amd.metapath, K0) against scipy on the same host, in the same process.

One JSON line per (preset, meta-path):
  gpu_ms        the whole metapath_graph call (relation transposes included: every timed call gets fresh relation
                objects), HIP events around it, 2 warm-ups, median of --reps (gpu_ms_all: every rep);
  scipy_s       the host preprocessing it replaces: the boolean sparse products of the chain left to right (the
                reverse hops as transposes), + I, indices sorted -- single-threaded scipy; scipy_sym_s the same
                product in the H Hᵀ form the GPU uses for palindromes;
  nnz, candidates = sum of the row bounds ub over every product of the call, products = their number;
  bytes_model   what the kernels must move: per product the candidate columns read twice (count + fill, 4 B each;
                a long row once per bit-map tile), the A entries and B row pointers behind them (4 + 16 B per A
                entry, three passes) and the per-row words (row list, bounds, counts, row pointers: 48 B per row),
                plus 4 B per output entry;
  exact         GPU output == scipy output (row pointers and columns, bit for bit).
--sweep: the GPU time alone over short-row bounds S x bit-map tiles (ops.SPGEMM_SHORT / SPGEMM_TILE).
--weights: per (preset, meta-path) the boolean call beside the weighted ones, same process, same median: bool_ms,
count_ms (weights="count"), pathsim_ms, pathsim_topk_ms (weights="pathsim", top_k=--top-k), count_over_bool, and
scipy_count_s = scipy's int64 product of the same chain (+ the stored diagonal, indices sorted), count_exact = the GPU
counts equal it, count_vs_scipy = scipy_count_s / count_ms.
--sample: the sampler (metapath.metapath_sample, han_metapath_walk_*) -- per DBLP-like hub meta-path sample_ms
(--walks, --fanout, weights="prob") beside pathsim_topk_ms of the same process and median, and recall@W for W = 64 / 256 /
1024: the share of the exact `fanout` strongest neighbours by random-walk transition probability (scipy on the host: the
product of the row-normalised relations, ties to the smaller column) that the sampled rows hold; for the hub preset
(10^6 authors, APCPA never formed) sample_ms at --walks / --hub-fanout, nnz, reads_per_pass = 2 x rows x walks x hops
(row pointers and the drawn entry of every hop; count and fill are a pass each), and -- unless --no-train -- epochs/s of
HANTrainer on four such graphs beside the regular SYN-1M graphs of bench.py in the same process.

    python tools/metapath_bench.py [--out FILE]
    python tools/metapath_bench.py --sweep [--out FILE]
    python tools/metapath_bench.py --no-scipy            # GPU only (the rocprofv3 run)
    python tools/metapath_bench.py --weights [--out FILE]
    python tools/metapath_bench.py --weights --no-scipy --presets pap-3m --reps 1     # (the rocprofv3 run)
    python tools/metapath_bench.py --sample --presets dblp-like,hub-1m [--out FILE]
    python tools/metapath_bench.py --sample --no-scipy --no-train --presets hub-1m --reps 1   # (the rocprofv3 run)
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from han_amd import metapath, ops, synth  # noqa: E402
from han_amd.graph import CSRGraph  # noqa: E402

PRESETS = {"dblp-like": ("APA", "APCPA", "APTPA"), "pap-3m": ("PAP",), "hub-1m": ("APCPA",)}


def fresh(rel):
    """New relation objects over the same device arrays: no cached transposes."""
    return {k: CSRGraph(g.rowptr, g.colidx, g.n_cols, validate=False) for k, g in rel.items()}


def gpu_time(rel, mp, reps, build=metapath.metapath_graph, **kw):
    ts, out = [], None
    for i in range(2 + reps):
        r = fresh(rel)
        out = None
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = build(r, mp, **kw)
        e1.record()
        torch.cuda.synchronize()
        if i >= 2:
            ts.append(e0.elapsed_time(e1))
    return out, ts


def stats_of(rel, mp):
    ops.SPGEMM_STATS = []
    try:
        metapath.metapath_graph(fresh(rel), mp)
        torch.cuda.synchronize()
        st = [{k: (int(v) if isinstance(v, torch.Tensor) else v) for k, v in d.items()} for d in ops.SPGEMM_STATS]
    finally:
        ops.SPGEMM_STATS = None
    tiles = -(-max(d["cols"] for d in st) // ops.SPGEMM_TILE)
    cand = sum(d["candidates"] for d in st)
    model = sum(8 * d["candidates"] + 60 * d["nnz_a"] + 48 * d["rows"] + 4 * d["nnz"] for d in st)
    return dict(products=len(st), candidates=cand, n_long=[d["n_long"] for d in st], bytes_model=model,
                max_tiles=tiles)


def to_scipy(g):
    return sp.csr_matrix((np.ones(g.nnz, dtype=bool), g.colidx.cpu().numpy(), g.rowptr.cpu().numpy()),
                         shape=(g.n_rows, g.n_cols))


def scipy_build(host, hops, n, sym):
    t0 = time.perf_counter()
    if sym is not None:
        h = host[hops[0][0]]
        for key, _ in hops[1:sym]:
            h = h @ host[key]
        m = h @ h.T.tocsr()
    else:
        m = None
        for key, t in hops:
            r = host[key].T.tocsr() if t else host[key]
            m = r if m is None else m @ r
    m = sp.csr_matrix(m + sp.identity(n, dtype=bool, format="csr"))
    m.sort_indices()
    return m, time.perf_counter() - t0


def scipy_count(host, hops, n):
    """scipy's int64 product of the chain left to right with every (i, i) stored (0 without an instance), indices
    sorted: (matrix, seconds)."""
    ones = {k: sp.csr_matrix(m, dtype=np.int64) for k, m in host.items()}
    t0 = time.perf_counter()
    m = None
    for key, t in hops:
        r = ones[key].T.tocsr() if t else ones[key]
        m = r if m is None else m @ r
    m = sp.csr_matrix(m + sp.identity(n, dtype=np.int64, format="csr"))
    m.sort_indices()
    dt = time.perf_counter() - t0
    m.data -= m.indices == np.repeat(np.arange(n), np.diff(m.indptr))
    return m, dt


def weights_line(rel, host, preset, mp, plan, reps, top_k):
    d = dict(preset=preset, metapath=mp, form="H Ht" if plan["split"] is not None else "left to right", top_k=top_k)
    for name, kw in (("bool", {}), ("count", dict(weights="count")), ("pathsim", dict(weights="pathsim")),
                     ("pathsim_topk", dict(weights="pathsim", top_k=top_k))):
        g, ts = gpu_time(rel, mp, reps, **kw)
        d[name + "_ms"] = round(float(np.median(ts)), 4)
        d[name + "_ms_all"] = [round(t, 4) for t in ts]
        d["nnz_topk" if name == "pathsim_topk" else "nnz"] = g.nnz
        if name == "count" and host is not None:
            ref, dt = scipy_count(host, plan["hops"], g.n_rows)
            d["count_exact"] = bool(np.array_equal(g.rowptr.cpu().numpy(), ref.indptr.astype(np.int64)) and
                                    np.array_equal(g.colidx.cpu().numpy(), ref.indices.astype(np.int32)) and
                                    np.array_equal(g.values.cpu().numpy(), ref.data.astype(np.float32)))
            d["scipy_count_s"] = round(dt, 3)
            del ref
        del g
        torch.cuda.empty_cache()
    d["count_over_bool"] = round(d["count_ms"] / d["bool_ms"], 2)
    if "scipy_count_s" in d:
        d["count_vs_scipy"] = round(d["scipy_count_s"] * 1e3 / d["count_ms"], 1)
    return d


def exact_top(host, hops, fanout):
    """Per row the `fanout` off-diagonal columns of largest random-walk transition probability (the product of the
    row-normalised relations along `hops`, float64, ties to the smaller column): a list of int arrays."""
    p = None
    for key, t in hops:
        m = sp.csr_matrix(host[key].T if t else host[key], dtype=np.float64)
        deg = np.asarray(m.sum(1)).ravel()
        m = sp.diags(np.divide(1.0, deg, out=np.zeros_like(deg), where=deg > 0)) @ m
        p = m if p is None else p @ m
    p = sp.csr_matrix(p)
    p.sort_indices()
    top = []
    for i in range(p.shape[0]):
        cols, vals = p.indices[p.indptr[i]:p.indptr[i + 1]], p.data[p.indptr[i]:p.indptr[i + 1]]
        off = cols != i
        cols, vals = cols[off], vals[off]
        top.append(cols[np.lexsort((cols, -vals))[:fanout]])
    return top


def recall(g, top):
    rp, ci = g.rowptr.cpu().numpy(), g.colidx.cpu().numpy()
    hit = sum(np.intersect1d(ci[rp[i]:rp[i + 1]], t, assume_unique=True).size for i, t in enumerate(top))
    return hit / max(1, sum(t.size for t in top))


def epochs_per_s(x, graphs, labels, train_mask, val_mask, dev, warmup=3, steps=30):
    """bench.py's model and trainer settings (eager, one stream) on `graphs`: epochs per second."""
    from han_amd.gat import HeteGAT_multi
    from han_amd.trainer import HANTrainer
    model = HeteGAT_multi().build(len(graphs), x.shape[1], 4, (8,), (8, 1), 128, device=dev,
                                  generator=torch.Generator().manual_seed(0))
    tr = HANTrainer(model, [x] * len(graphs), graphs, labels, train_mask, val_mask, lr=0.005, l2_coef=0.001,
                    attn_drop=0.6, ffd_drop=0.6)
    for _ in range(warmup):
        tr.epoch()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        last = tr.epoch()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert np.isfinite(float(last[0]))
    return steps / dt


def sample_line(rel, host, preset, mp, plan, args, dev):
    hub = preset == "hub-1m"
    fanout = args.hub_fanout if hub else args.fanout
    n = plan["sizes"][mp[0]]
    d = dict(preset=preset, metapath=mp, rows=n, walks=args.walks, fanout=fanout)
    g, ts = gpu_time(rel, mp, args.reps, build=metapath.metapath_sample, walks=args.walks, fanout=fanout,
                     weights="prob")
    d.update(sample_ms=round(float(np.median(ts)), 4), sample_ms_all=[round(t, 4) for t in ts], nnz=g.nnz,
             max_row=int(g.degrees().max()), reads_per_pass=2 * n * args.walks * len(plan["hops"]))
    del g
    if not hub:
        g, ts = gpu_time(rel, mp, args.reps, weights="pathsim", top_k=fanout)
        d.update(pathsim_topk_ms=round(float(np.median(ts)), 4), pathsim_topk_ms_all=[round(t, 4) for t in ts],
                 nnz_pathsim_topk=g.nnz)
        d["pathsim_topk_over_sample"] = round(d["pathsim_topk_ms"] / d["sample_ms"], 2)
        del g
        if host is not None:
            top = exact_top(host, plan["hops"], fanout)
            for w in (64, 256, 1024):
                s = metapath.metapath_sample(rel, mp, walks=w, fanout=min(fanout, w))
                d[f"recall_at_{w}"] = round(recall(s, top), 4)
    elif not args.no_train:
        graphs = [metapath.metapath_sample(rel, mp, walks=args.walks, fanout=fanout, seed=s) for s in range(4)]
        wl = synth.make_workload("syn-1m", device=dev)
        assert wl["n"] == n
        d["epochs_per_s_sampled"] = round(epochs_per_s(wl["x"], graphs, wl["labels"], wl["train_mask"], wl["val_mask"],
                                                       dev), 2)
        d["nnz_train_graphs"] = sum(g.nnz for g in graphs)
        del graphs
        torch.cuda.empty_cache()
        d["epochs_per_s_syn1m"] = round(epochs_per_s(wl["x"], wl["graphs"], wl["labels"], wl["train_mask"],
                                                     wl["val_mask"], dev), 2)
        d["nnz_syn1m"] = sum(g.nnz for g in wl["graphs"])
    torch.cuda.empty_cache()
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--presets", default="dblp-like,pap-3m")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--weights", action="store_true")
    ap.add_argument("--top-k", type=int, default=32)
    ap.add_argument("--sample", action="store_true")
    ap.add_argument("--walks", type=int, default=256)
    ap.add_argument("--fanout", type=int, default=32)
    ap.add_argument("--hub-fanout", type=int, default=49)
    ap.add_argument("--no-train", action="store_true")
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    out = open(args.out, "w") if args.out else None

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    for preset in args.presets.split(","):
        rel, sizes = synth.hetero_relations(preset, device=dev)
        host = None if (args.no_scipy or args.sweep or preset == "hub-1m") else {k: to_scipy(g) for k, g in rel.items()}
        for mp in PRESETS[preset]:
            plan = metapath.plan(rel, mp)
            if args.sample:
                if mp != "APA":                # (the hub meta-paths: APA is small as a product)
                    emit(sample_line(rel, host, preset, mp, plan, args, dev))
                continue
            if args.sweep:
                for S in (256, 1024, 4096):
                    for T in (1 << 15, 1 << 17, 1 << 19):
                        ops.SPGEMM_SHORT, ops.SPGEMM_TILE = S, T
                        _, ts = gpu_time(rel, mp, args.reps)
                        emit(dict(preset=preset, metapath=mp, short_max=S, tile_cols=T,
                                  gpu_ms=round(float(np.median(ts)), 4), gpu_ms_all=[round(t, 4) for t in ts]))
                continue
            if args.weights:
                emit(weights_line(rel, host, preset, mp, plan, args.reps, args.top_k))
                continue
            g, ts = gpu_time(rel, mp, args.reps)
            med = float(np.median(ts))
            st = stats_of(rel, mp)
            d = dict(preset=preset, metapath=mp, form="H Ht" if plan["split"] is not None else "left to right",
                     short_max=ops.SPGEMM_SHORT, tile_cols=ops.SPGEMM_TILE, rows=g.n_rows, nnz=g.nnz,
                     gpu_ms=round(med, 4), gpu_ms_all=[round(t, 4) for t in ts], **st,
                     model_GBps=round(st["bytes_model"] / med / 1e6, 1))
            if host is not None:
                ref, t_chain = scipy_build(host, plan["hops"], g.n_rows, None)
                d["exact"] = bool(np.array_equal(g.rowptr.cpu().numpy(), ref.indptr.astype(np.int64)) and
                                  np.array_equal(g.colidx.cpu().numpy(), ref.indices.astype(np.int32)))
                del ref
                d["scipy_s"] = round(t_chain, 3)
                if plan["split"] is not None and plan["split"] > 1:      # (split 1: the chain IS H Hᵀ)
                    _, t_sym = scipy_build(host, plan["hops"], g.n_rows, plan["split"])
                    d["scipy_sym_s"] = round(t_sym, 3)
                d["speedup_vs_scipy"] = round(t_chain * 1e3 / med, 1)
            emit(d)
            del g
            torch.cuda.empty_cache()
        del rel, host
    if out:
        out.close()


if __name__ == "__main__":
    main()
