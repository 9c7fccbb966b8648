#!/usr/bin/env python3
"""Time the semantic attention with one weight per meta-path (han_sem_attn_mean_fwd / _bwd, han.pdf eq. 7-9) beside the
per-node kernels (han_sem_attn_fwd / han_sem_attn_bwd) of the same tree, and a SYN-1M epoch of HANTrainer in either mode
(DESIGN.md section 5, round 28).

    python tools/sem_metapath_bench.py --out FILE.jsonl [--rounds 3] [--no-epoch]      # the driver
    python tools/sem_metapath_bench.py --side node|metapath                            # one process of it
    python tools/sem_metapath_bench.py --epoch-side node|node-full|metapath            # one epoch process of it

The protocol is that of tools/multilabel_bench.py: the driver starts one process per side and round, alternating
(node, metapath, node, ...); each process times, at N = 10^6, P = 4 and (D, A) in {(64, 128), (64, 64), (128, 128)} --
the first is the SYN-1M K3 shape --, the forward and the backward: 20 calls after 5 warm-ups, device events around each
call (a call is every launch of the entry: for the new forward the score pass, the finishing block and the combine
pass; for the new backward the d beta pass, the finishing block, the main pass per slice and the slab reduction),
median; the driver takes the median of the process medians.  Beside each time stands the byte floor of the new form --
forward 2 |M| + |Z|, backward 2 |M| + |dZ| + |dM| -- as bytes and as the time those bytes take at the 8 TB/s HBM peak,
and the fraction of that floor the call achieves.  The epoch lines: "node" is the default trainer, "node-full" the node
mode with live_forward=False, live_backward=False (every row visited, as the published form has to), "metapath" the
new mode."""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, P = 1_000_000, 4
SHAPES = ((64, 128), (64, 64), (128, 128))      # (D, A)
HBM_PEAK_GBS = 8000.0                           # MI355X: 8.0 TB/s


def floors(D):
    """Byte floors of the new form at (N, P, D): forward 2 |M| + |Z|, backward 2 |M| + |dZ| + |dM|."""
    m, z = 4 * N * P * D, 4 * N * D
    return {"fwd": 2 * m + z, "bwd": 2 * m + z + m}


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
    res = {}
    for D, A in SHAPES:
        M = torch.randn((N, P, D), generator=g, device=dev)
        dZ = torch.randn((N, D), generator=g, device=dev)
        w = torch.randn((D, A), generator=g, device=dev) * 0.1
        b = torch.randn((A,), generator=g, device=dev) * 0.1
        u = torch.randn((A,), generator=g, device=dev) * 0.1
        fwd, bwd = (ops.sem_attn_mean_fwd, ops.sem_attn_mean_bwd) if side == "metapath" else (ops.sem_attn_fwd, ops.sem_attn_bwd)
        out = (torch.empty((N, D), device=dev), torch.empty((P,) if side == "metapath" else (N, P), device=dev))
        res[f"D={D} A={A} fwd"] = _events(lambda: fwd(M, w, b, u, out=out), 5, 20)
        beta = out[1]
        grads = (torch.empty_like(w), torch.empty_like(b), torch.empty_like(u))
        keep = []

        def back():      # dM is allocated by the op: keep one alive so that the allocator hands the same block back
            keep[:] = [bwd(M, w, b, u, beta, dZ, out=grads)]
        res[f"D={D} A={A} bwd"] = _events(back, 5, 20)
        del M, dZ, keep, out
        torch.cuda.empty_cache()
    return res


def side_epoch(side):
    import torch
    from han_amd import synth
    from han_amd.gat import HeteGAT_multi
    from han_amd.trainer import HANTrainer
    dev = torch.device("cuda:0")
    wl = synth.make_workload("syn-1m", device=dev)
    model = HeteGAT_multi().build(wl["p"], wl["f"], wl["c"], (8,), (8, 1), 128, device=dev,
                                  generator=torch.Generator().manual_seed(2),
                                  semantic="metapath" if side == "metapath" else "node")
    kw = dict(live_forward=False, live_backward=False) if side == "node-full" else {}
    tr = HANTrainer(model, [wl["x"]] * wl["p"], wl["graphs"], wl["labels"], wl["train_mask"], wl["val_mask"], **kw)
    out = []

    def epoch():
        out[:] = [tr.epoch()]
    ms = _events(epoch, 3, 10)
    res = {"epoch_ms": ms, "scalars": [float(v) for v in out[0]], "live_forward": tr.live_forward,
           "live_backward": tr.live_backward}
    if side == "metapath":
        with torch.no_grad():
            _, att = model.semantic(model.node_level(tr.xs, tr.graphs, 0.0, 0.0, False, 1))
        res["beta"] = [float(v) for v in att[0]]
    return res


def _run(args, flag, side):
    cmd = [sys.executable, os.path.join(HERE, "tools", "sem_metapath_bench.py"), flag, side]
    p = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ), timeout=args.timeout)
    if p.returncode != 0:
        sys.stderr.write(p.stdout + p.stderr)
        raise SystemExit(p.returncode)
    return json.loads(p.stdout.strip().splitlines()[-1])


def driver(args):
    per = {"node": [], "metapath": []}
    for r in range(args.rounds):
        for side in ("node", "metapath"):
            per[side].append(_run(args, "--side", side))
            print(f"round {r} {side}: done", flush=True)
    lines = []
    for key in per["node"][0]:
        a = [x[key] for x in per["node"]]
        b = [x[key] for x in per["metapath"]]
        D = int(key.split()[0][2:])
        fl = floors(D)[key.split()[-1]]
        floor_ms = fl / (HBM_PEAK_GBS * 1e6)
        lines.append({"what": f"N={N} P={P} {key}", "node_ms": statistics.median(a), "metapath_ms": statistics.median(b),
                      "ratio": statistics.median(b) / statistics.median(a), "byte_floor": fl,
                      "floor_ms_at_8TBs": round(floor_ms, 4), "achieved_fraction": round(floor_ms / statistics.median(b), 4),
                      "node_all": a, "metapath_all": b})
    if not args.no_epoch:
        ep = {"node": [], "node-full": [], "metapath": []}
        for r in range(args.rounds):
            for side in ep:
                ep[side].append(_run(args, "--epoch-side", side))
                print(f"round {r} epoch {side}: done", flush=True)
        med = {s: statistics.median(x["epoch_ms"] for x in v) for s, v in ep.items()}
        lines.append({"what": "SYN-1M epoch", "node_default_ms": med["node"], "node_every_row_ms": med["node-full"],
                      "metapath_ms": med["metapath"], "ratio_to_default": med["metapath"] / med["node"],
                      "ratio_to_every_row": med["metapath"] / med["node-full"],
                      "all": {s: [x["epoch_ms"] for x in v] for s, v in ep.items()},
                      "node_default_live": [ep["node"][-1]["live_forward"], ep["node"][-1]["live_backward"]],
                      "metapath_scalars": ep["metapath"][-1]["scalars"], "metapath_beta": ep["metapath"][-1]["beta"]})
    with open(args.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
            print(json.dumps(line))
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--side", choices=("node", "metapath"))
    ap.add_argument("--epoch-side", choices=("node", "node-full", "metapath"))
    ap.add_argument("--no-epoch", action="store_true")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.side is None and args.epoch_side is None:
        if not args.out:
            ap.error("the driver needs --out")
        return driver(args)
    sys.path.insert(0, HERE)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures, it has no fallback")
    print(json.dumps(side_epoch(args.epoch_side) if args.epoch_side else side_entry(args.side)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
