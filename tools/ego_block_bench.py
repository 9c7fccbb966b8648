#!/usr/bin/env python3
"""Ego blocks at SYN-1M, one MI355X, one process: what a block costs to cut and what it saves.

For each workload (syn-1m: 50 neighbours per row; syn-1m-skew: power-law rows, a few of them very long), P = 4
meta-path graphs, B seeds drawn from a seeded permutation, and `hops` layers:

  (a) extraction   minibatch.ego_block (han_ego_* kernels) next to torch_block below -- the same block built from
                   torch index ops alone --, alternating, each call between two device synchronisations (both sides
                   read sizes on the host, so the host clock around a synchronised call is the time a user waits);
                   the two blocks are compared bit for bit first;
  (b) inference    minibatch.predict of the B rows (one block) next to ONE full-graph eval forward (what answers a
                   query today), for a model of `hops` node-attention layers;
  (c) training     MiniBatchTrainer.train_step on a batch of B next to HANTrainer.train_step on the whole graph
                   (dropout 0.6 / 0.6 on both).

With --fanout F every (workload, B, hops) measures instead, in the same process and the same alternating windows, the
SAMPLED block (ego_block(fanout=F, seed=): at most F neighbours per row, graph and hop, han_ego_sample_* kernels) next
to the unsampled block and the full graph: extraction (sampled | whole), predict (sampled | whole | one full-graph eval
forward) and the training step (sampled | whole | HANTrainer.train_step); the line also holds both blocks' sizes and
whether entries <= kept rows x F + self entries + rim rows holds for every block graph.  Default --out then:
profiles/r18_ego_sample_bench.jsonl.

One JSON line per (workload, B, hops) with the block sizes (n_b, entries per graph) and median / min / max
milliseconds over `reps` alternating windows after a warm-up; lines are appended as they are measured.

    python tools/ego_block_bench.py [--out profiles/r16_ego_block_bench.jsonl] [--workloads syn-1m,syn-1m-skew]
                                    [--batches 1024,8192] [--hops 1,2] [--reps 5] [--n N] [--append] [--fanout F]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from han_amd import csr, minibatch, ops, synth  # noqa: E402
from han_amd.gat import HeteGAT_multi  # noqa: E402
from han_amd.graph import CSRGraph  # noqa: E402
from han_amd.trainer import HANTrainer  # noqa: E402


def torch_block(graphs, seeds, hops):
    """minibatch.ego_block from torch ops alone (nonzero / repeat_interleave / index ops): the same EgoBlock."""
    n, dev = graphs[0].n_rows, graphs[0].device
    s = seeds.to(torch.int64)
    level = torch.full((n,), -1, dtype=torch.int32, device=dev)
    level[s] = 0
    degs = [g.degrees() for g in graphs]
    for h in range(hops):
        frontier = torch.nonzero(level == h).flatten()
        for g, deg in zip(graphs, degs):
            cols = g.colidx[csr.ragged_index(g.rowptr[frontier], deg[frontier])].long()
            level[cols[level[cols] < 0]] = h + 1
    nodes = torch.nonzero(level >= 0).flatten()
    n_b = nodes.numel()
    local = torch.full((n,), -1, dtype=torch.int32, device=dev)
    local[nodes] = torch.arange(n_b, dtype=torch.int32, device=dev)
    kept = level[nodes] < hops
    rows_b = torch.arange(n_b, device=dev)
    out = []
    for g, deg in zip(graphs, degs):
        deg_b = torch.where(kept, deg[nodes], torch.ones_like(nodes))
        rowptr = csr.scan(deg_b)
        src = csr.ragged_index(g.rowptr[nodes[kept]], deg_b[kept])
        dst = csr.ragged_index(rowptr[:-1][kept], deg_b[kept])
        colidx = torch.empty(int(rowptr[-1]), dtype=torch.int32, device=dev)
        colidx[dst] = local[g.colidx[src].long()]
        colidx[rowptr[:-1][~kept]] = rows_b[~kept].to(torch.int32)
        values = None
        if g.values is not None:
            values = torch.ones(colidx.numel(), dtype=torch.float32, device=dev)
            values[dst] = g.values[src]
        out.append(CSRGraph(rowptr, colidx, n_b, validate=False, values=values))
    return minibatch.EgoBlock(nodes=nodes, level=level[nodes], seed_pos=local[s].long(), graphs=out, n=n)


def same_block(a, b):
    ok = torch.equal(a.nodes, b.nodes) and torch.equal(a.level, b.level) and torch.equal(a.seed_pos, b.seed_pos)
    for g, h in zip(a.graphs, b.graphs):
        ok = ok and torch.equal(g.rowptr, h.rowptr) and torch.equal(g.colidx, h.colidx)
    return bool(ok)


def timed(sides, reps, warmup=2):
    """sides: {name: fn}; alternating windows, one call each, between device synchronisations; milliseconds."""
    for fn in sides.values():
        for _ in range(warmup):
            fn()
    ts = {k: [] for k in sides}
    for _ in range(reps):
        for k, fn in sides.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts[k].append((time.perf_counter() - t0) * 1e3)
    return {k: dict(median=round(sorted(v)[len(v) // 2], 3), min=round(min(v), 3), max=round(max(v), 3))
            for k, v in ts.items()}


def block_sizes(blk, hops):
    return dict(n_b=int(blk.nodes.numel()), nnz=[g.nnz for g in blk.graphs], rim=int((blk.level == hops).sum()))


def fanout_bound_holds(blk, hops, fanout):
    """entries <= kept rows x fanout + self entries of the kept rows + one per rim row, for every block graph."""
    kept = blk.level < hops
    n_kept, n_rim = int(kept.sum()), int((~kept).sum())
    ok = True
    for g in blk.graphs:
        rows = torch.repeat_interleave(torch.arange(g.n_rows, device=g.device), g.degrees())
        n_self = int(((g.colidx == rows) & kept[rows]).sum())
        ok = ok and g.nnz <= n_kept * fanout + n_self + n_rim
    return bool(ok)


def sampled_line(args, name, wl, model, full, full_eval, graphs, seeds, B, hops):
    """The --fanout line of one (workload, B, hops): sampled block | unsampled block | full graph, one job."""
    f, P = args.fanout, wl["p"]
    xs, labels = [wl["x"]] * P, wl["labels"]
    mini = {k: minibatch.MiniBatchTrainer(model, xs, graphs, labels, wl["train_mask"], wl["val_mask"], batch_size=B,
                                          seed=1, fanout=fo) for k, fo in (("sampled", f), ("whole", None))}
    blk = minibatch.ego_block(graphs, seeds, hops, fanout=f, seed=1)
    sizes = dict(sampled=block_sizes(blk, hops), bound_holds=fanout_bound_holds(blk, hops, f))
    reproducible = same_block(blk, minibatch.ego_block(graphs, seeds, hops, fanout=f, seed=1))
    blk = minibatch.ego_block(graphs, seeds, hops)
    sizes["whole"] = block_sizes(blk, hops)
    del blk
    t = {}
    t.update({"extract_" + k: v for k, v in timed(
        {"sampled": lambda: minibatch.ego_block(graphs, seeds, hops, fanout=f, seed=1),
         "whole": lambda: minibatch.ego_block(graphs, seeds, hops)}, args.reps).items()})
    t.update({"infer_" + k: v for k, v in timed(
        {"sampled": lambda: minibatch.predict(model, full.xs, graphs, seeds, batch_size=B, fanout=f, seed=1),
         "whole": lambda: minibatch.predict(model, full.xs, graphs, seeds, batch_size=B),
         "full": full_eval}, args.reps).items()})
    t.update({"train_" + k: v for k, v in timed(
        {"sampled": lambda: mini["sampled"].train_step(seeds), "whole": lambda: mini["whole"].train_step(seeds),
         "full": full.train_step}, args.reps).items()})
    return dict(tool="ego_block_bench", mode="fanout", workload=name, N=wl["n"], P=P, B=B, hops=hops, fanout=f, **sizes,
                full_nnz=[g.nnz for g in graphs], reproducible=reproducible, windows=args.reps, ms=t,
                train_sampled_vs_whole=round(t["train_whole"]["median"] / t["train_sampled"]["median"], 3),
                train_sampled_vs_full=round(t["train_full"]["median"] / t["train_sampled"]["median"], 3),
                device=torch.cuda.get_device_name(0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default: profiles/r16_ego_block_bench.jsonl, with --fanout "
                                                "profiles/r18_ego_sample_bench.jsonl")
    ap.add_argument("--fanout", type=int, default=None, help="measure sampled blocks of this fan-out per graph and hop")
    ap.add_argument("--workloads", default="syn-1m,syn-1m-skew")
    ap.add_argument("--batches", default="1024,8192")
    ap.add_argument("--hops", default="1,2")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=None, help="override the node count (rehearsals)")
    ap.add_argument("--append", action="store_true", help="add to --out instead of starting it afresh")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join("profiles", "r18_ego_sample_bench.jsonl" if args.fanout else "r16_ego_block_bench.jsonl")
    if not torch.cuda.is_available():
        raise SystemExit("ego_block_bench needs a GPU: a CPU run gives no timing")
    dev = torch.device("cuda:0")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if not args.append:
        open(args.out, "w").close()
    for name in args.workloads.split(","):
        wl = synth.make_workload(name, device=dev, n_override=args.n)
        graphs, x, n = wl["graphs"], wl["x"], wl["n"]
        perm = torch.randperm(n, generator=torch.Generator().manual_seed(17)).to(dev)
        for hops in (int(v) for v in args.hops.split(",")):
            hid, heads = (8,) * hops, (8,) * hops + (1,)
            model = HeteGAT_multi().build(wl["p"], wl["f"], wl["c"], hid, heads, 128, device=dev,
                                          generator=torch.Generator().manual_seed(3))
            full = HANTrainer(model, [x] * wl["p"], graphs, wl["labels"], wl["train_mask"], wl["val_mask"])

            def full_eval():
                with torch.no_grad():
                    M = model.node_level(full.xs, full.graphs, 0.0, 0.0, False, ops.ACT_ELU)
                    return model.classify(model.semantic(M)[0])

            for B in (int(v) for v in args.batches.split(",")):
                seeds = perm[:B].contiguous()
                if args.fanout:
                    line = sampled_line(args, name, wl, model, full, full_eval, graphs, seeds, B, hops)
                    print(json.dumps(line), flush=True)
                    with open(args.out, "a") as fh:
                        fh.write(json.dumps(line) + "\n")
                    torch.cuda.empty_cache()
                    continue
                mini = minibatch.MiniBatchTrainer(model, [x] * wl["p"], graphs, wl["labels"], wl["train_mask"],
                                                  wl["val_mask"], batch_size=B, seed=1)
                blk = minibatch.ego_block(graphs, seeds, hops)
                equal = same_block(blk, torch_block(graphs, seeds, hops))
                sizes = dict(n_b=int(blk.nodes.numel()), nnz=[g.nnz for g in blk.graphs],
                             rim=int((blk.level == hops).sum()), full_nnz=[g.nnz for g in graphs])
                del blk
                t = {}
                t.update({"extract_" + k: v for k, v in timed(
                    {"hip": lambda: minibatch.ego_block(graphs, seeds, hops),
                     "torch": lambda: torch_block(graphs, seeds, hops)}, args.reps).items()})
                t.update({"infer_" + k: v for k, v in timed(
                    {"block": lambda: minibatch.predict(model, full.xs, graphs, seeds, batch_size=B),
                     "full": full_eval}, args.reps).items()})
                t.update({"train_" + k: v for k, v in timed(
                    {"block": lambda: mini.train_step(seeds), "full": full.train_step}, args.reps).items()})
                line = dict(tool="ego_block_bench", workload=name, N=n, P=wl["p"], B=B, hops=hops, **sizes,
                            torch_block_equal=equal, windows=args.reps, ms=t,
                            extract_speedup=round(t["extract_torch"]["median"] / t["extract_hip"]["median"], 3),
                            infer_speedup=round(t["infer_full"]["median"] / t["infer_block"]["median"], 3),
                            train_speedup=round(t["train_full"]["median"] / t["train_block"]["median"], 3),
                            device=torch.cuda.get_device_name(0))
                print(json.dumps(line), flush=True)
                with open(args.out, "a") as fh:
                    fh.write(json.dumps(line) + "\n")
                del mini
                torch.cuda.empty_cache()
            del full, model
            torch.cuda.empty_cache()
        del wl, graphs, x
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
