#!/usr/bin/env python3
"""Time the multi-label classifier entry (han_classifier_multilabel) against the softmax one (han_classifier_loss /
han_classifier_loss_live), and a SYN-1M epoch under either objective.

    python tools/multilabel_bench.py --out FILE.jsonl [--softmax-tree DIR] [--rounds 5]      # the driver
    python tools/multilabel_bench.py --side softmax|sigmoid [--epoch]                         # one process of it

The driver starts one process per side and round, alternating (softmax, sigmoid, softmax, ...); `--softmax-tree` names
another checkout whose han_amd the softmax processes import -- the parent commit's, built there -- so that the
comparison is against the parent's kernels; by default both sides run this tree.  Each process times, at N = 10^6,
D = 64, C in {4, 16, 64}, the forward alone and with the backward, over every row and over a row list of 10 % of the
rows (every 10th row; the mask on the same rows in all four): 20 calls after 5 warm-ups, device events around each
call (a call is the kernel, its slab reduction and, for the sigmoid side, the finishing kernel), median.  Both sides
move the same bytes -- Z in, logits and dZ out -- and differ in the per-class work: C exponentials and one logarithm
per row for softmax, C exponentials, C logarithms and C divisions (with the backward) for sigmoid.  The driver writes
one line per (shape, mode) with the medians over the rounds and their ratio, and with `--epoch` one line for the
SYN-1M epoch of HANTrainer (C = 16 label planes, objective="sigmoid") beside the softmax epoch (the workload's own
class ids; C = 16 too) of the same job.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, D, HC = 1_000_000, 64, 1
CLASSES = (4, 16, 64)


def _events(fn, warm, reps):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def side_entry(side):
    import torch
    from han_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    Z = torch.randn((N, D), generator=g, device=dev)
    live = torch.arange(0, N, 10, dtype=torch.int32, device=dev)
    mask = torch.zeros(N, dtype=torch.uint8, device=dev)
    mask[live.long()] = 1
    res = {}
    for C in CLASSES:
        Wc = torch.randn((HC, D, C), generator=g, device=dev) * 0.25
        bc = torch.zeros((HC, C), device=dev)
        if side == "sigmoid":
            labels = ops.pack_label_bits((torch.rand((N, C), generator=g, device=dev) < 0.3).to(torch.uint8))
            call = ops.classifier_multilabel
        else:
            labels = torch.randint(0, C, (N,), generator=g, device=dev, dtype=torch.int32)
            call = ops.classifier_loss
        for bwd in (False, True):
            for rows, lv in (("all", None), ("list10", live)):
                res[f"C={C} {'fwd+bwd' if bwd else 'fwd'} {rows}"] = _events(
                    lambda: call(Z, Wc, bc, labels, mask, 1.0 / live.numel(), backward=bwd, live=lv), 5, 20)
    return res


def side_epoch(side):
    import torch
    from han_amd import synth
    from han_amd.gat import HeteGAT_multi
    from han_amd.trainer import HANTrainer
    dev = torch.device("cuda:0")
    wl = synth.make_workload("syn-1m", device=dev)
    C = 16
    com = torch.randint(0, C, (wl["n"],), generator=torch.Generator().manual_seed(3), dtype=torch.int32).to(dev)
    kw = {}
    if side == "sigmoid":
        labels, kw = synth.multilabel_labels(com, C, seed=3), dict(objective="sigmoid")
    else:
        labels = com
    model = HeteGAT_multi().build(wl["p"], wl["f"], C, (8,), (8, 1), 128, device=dev,
                                  generator=torch.Generator().manual_seed(2))
    tr = HANTrainer(model, [wl["x"]] * wl["p"], wl["graphs"], labels, wl["train_mask"], wl["val_mask"], **kw)
    out = []

    def epoch():
        out[:] = [tr.epoch()]
    ms = _events(epoch, 3, 10)
    return {"epoch_ms": ms, "scalars": [float(v) for v in out[0]]}


def driver(args):
    env = dict(os.environ)
    per = {"softmax": [], "sigmoid": []}
    for r in range(args.rounds):
        for side in ("softmax", "sigmoid"):
            tree = args.softmax_tree if (side == "softmax" and args.softmax_tree) else HERE
            cmd = [sys.executable, os.path.join(HERE, "tools", "multilabel_bench.py"), "--side", side, "--tree", tree]
            if args.epoch:
                cmd.append("--epoch")
            p = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=args.timeout)
            if p.returncode != 0:
                sys.stderr.write(p.stdout + p.stderr)
                return p.returncode
            per[side].append(json.loads(p.stdout.strip().splitlines()[-1]))
            print(f"round {r} {side}: done", flush=True)
    with open(args.out, "a") as f:
        if args.epoch:
            a = [x["epoch_ms"] for x in per["softmax"]]
            b = [x["epoch_ms"] for x in per["sigmoid"]]
            line = {"what": "SYN-1M epoch, C = 16", "softmax_ms": statistics.median(a), "sigmoid_ms": statistics.median(b),
                    "ratio": statistics.median(b) / statistics.median(a), "softmax_all": a, "sigmoid_all": b,
                    "sigmoid_scalars": per["sigmoid"][-1]["scalars"], "softmax_tree": args.softmax_tree or "this tree"}
            f.write(json.dumps(line) + "\n")
            print(json.dumps(line))
        else:
            for key in per["softmax"][0]:
                a = [x[key] for x in per["softmax"]]
                b = [x[key] for x in per["sigmoid"]]
                line = {"what": f"N={N} D={D} HC={HC} {key}", "softmax_ms": statistics.median(a),
                        "sigmoid_ms": statistics.median(b), "ratio": statistics.median(b) / statistics.median(a),
                        "softmax_all": a, "sigmoid_all": b, "softmax_tree": args.softmax_tree or "this tree"}
                f.write(json.dumps(line) + "\n")
                print(json.dumps(line))
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--side", choices=("softmax", "sigmoid"))
    ap.add_argument("--tree", default=HERE, help="(with --side) the checkout whose han_amd is imported")
    ap.add_argument("--softmax-tree", default=None)
    ap.add_argument("--epoch", action="store_true")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.side is None:
        if not args.out:
            ap.error("the driver needs --out")
        return driver(args)
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures, it has no fallback")
    print(json.dumps(side_epoch(args.side) if args.epoch else side_entry(args.side)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
