#!/usr/bin/env python3
"""The reference's experiment (``ex_acm3025.py``) on han_amd: load the ACM3025-style
``.mat`` (or, with no file, a synthetic graph of the same shape), train the 8-head HAN
full-graph with early stopping, restore the best weights, report the test metrics and the
KNN / KMeans scores of ``final_embed``.

    python examples/ex_acm3025.py [--mat ACM3025.mat] [--epochs 200] [--graph] [--eval-device gpu] [--sparse-features]
                                  [--batch-size B [--fanout 10 | --fanout 10,5]] [--multilabel]

Hyper-parameters are the reference's (ex_acm3025.py:16-31): lr 0.005, l2 0.001,
hid_units [8], n_heads [8, 1], dropout 0.6/0.6, patience 100, mp_att_size 128.
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from han_amd import SparseFeatures, evaluate, process, synth  # noqa: E402
from han_amd.gat import HeteGAT_multi  # noqa: E402
from han_amd.minibatch import MiniBatchTrainer  # noqa: E402
from han_amd.trainer import HANTrainer  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mat", default=None, help="ACM3025.mat-style file (keys label, feature, PAP, PLP, *_idx)")
    ap.add_argument("--epochs", type=int, default=200)
    ap.add_argument("--patience", type=int, default=100)
    ap.add_argument("--graph", action="store_true", help="replay the epoch from a hipGraph")
    ap.add_argument("--overlap-eval", action="store_true",
                    help="with --graph: validate the parameters of epoch k - 1 beside the training step of epoch k "
                         "(HANTrainer(overlap_eval=True)); the early-stopping rule then sees each pair one call later")
    ap.add_argument("--planted", action="store_true",
                    help="without --mat: a synthetic task WITH structure (communities) instead of the ACM-shaped "
                         "random-label workload, to watch the model learn")
    ap.add_argument("--sparse-features", action="store_true",
                    help="feed the features as a CSR matrix (han_amd.SparseFeatures): the first-layer projection then "
                         "visits the stored entries only; without --mat, a generated bag-of-words of the ACM shape")
    ap.add_argument("--batch-size", type=int, default=None, metavar="B",
                    help="train in mini-batches of B training nodes on the ego block of each batch "
                         "(han_amd.minibatch.MiniBatchTrainer) instead of one full-graph step per epoch")
    ap.add_argument("--fanout", default=None, metavar="F[,F...]",
                    help="with --batch-size: sample every step's block afresh, at most F neighbours per row and "
                         "meta-path (one number, or one per node-attention layer: the seeds' rows first)")
    ap.add_argument("--multilabel", action="store_true",
                    help="the reference's multi-label pair (masked sigmoid cross-entropy, micro-F1; "
                         "models/base_gattn.py:50-59,71-94) on the synthetic planted task: every node carries several "
                         "of 5 label planes (synth.multilabel_labels); reports micro-F1 per epoch and at the end")
    ap.add_argument("--semantic", choices=("node", "metapath"), default="node",
                    help="semantic attention: node = the softmax over the meta-paths per node (utils/layers.py:156); "
                         "metapath = the published form, one weight per meta-path from the node means of the scores "
                         "(han.pdf eq. 7-9): the P weights are printed with every reported epoch")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--eval-device", choices=("cpu", "gpu"), default="cpu",
                    help="where final_embed is scored: cpu = scikit-learn on the host, as the reference; gpu = the "
                         "evaluation kernels (the embeddings are not copied to the host)")
    ap.add_argument("--silhouette", action="store_true",
                    help="also report the silhouette score of the k-means labels (the data/exp.py form of my_Kmeans)")
    ap.add_argument("--tsne", metavar="PATH", default=None,
                    help="save the two-dimensional t-SNE coordinates of the scored embeddings and their labels as an .npz "
                         "(evaluate.tsne: scikit-learn exact t-SNE on the host, the han_tsne kernels with --eval-device gpu)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(args.seed)

    if args.multilabel and args.mat:
        ap.error("--multilabel runs on synthetic data (the ACM3025 file carries one label per node)")
    metric = "micro-F1" if args.multilabel else "acc"
    if args.mat:
        adj_list, fea_list, y_train, y_val, y_test, train_mask, val_mask, test_mask = process.load_data_mat(args.mat)
        graphs = [process.adj_to_graph(a, nhood=1, device=dev) for a in adj_list]      # == adj_to_bias's edge set
        if args.sparse_features:
            import scipy.sparse as sp
            conv = {}      # the meta-paths usually share one matrix: convert it once
            xs = [conv.setdefault(id(f), SparseFeatures.from_scipy(sp.csr_matrix(f), device=dev))
                  for f in fea_list[:len(graphs)]]
        else:
            xs = [torch.tensor(f, dtype=torch.float32, device=dev) for f in fea_list[:len(graphs)]]
        y = y_train + y_val + y_test
        labels = torch.tensor(y.argmax(1), dtype=torch.int32, device=dev)
        masks = [torch.tensor(m, device=dev) for m in (train_mask, val_mask, test_mask)]
        nb_classes = y.shape[1]
    elif args.planted or args.multilabel:
        wl = synth.planted_partition(3025, 3, 2, 64, deg_in=8, deg_out=2, noise=1.0, seed=args.seed, device=dev)
        graphs, xs = wl["graphs"], [wl["x"]] * wl["p"]
        labels, nb_classes = wl["labels"], wl["c"]
        masks = [wl["train_mask"], wl["val_mask"], wl["test_mask"]]
    else:
        wl = synth.make_workload("acm-like", device=dev)
        graphs, xs = wl["graphs"], [wl["x"]] * wl["p"]
        labels, nb_classes = wl["labels"], wl["c"]
        test = ~(wl["train_mask"].bool() | wl["val_mask"].bool())
        masks = [wl["train_mask"], wl["val_mask"], test]
        if args.sparse_features:      # ~1 % of the 1870 columns per row, a few words in most documents
            xs = [synth.bag_of_words(wl["n"], wl["f"], 20, seed=args.seed, device=dev)] * wl["p"]
    classes, n_groups = labels, nb_classes      # what the embeddings are scored against: one id per node
    if args.multilabel:
        labels, nb_classes = synth.multilabel_labels(classes, 5, seed=args.seed), 5
    objective = dict(objective="sigmoid" if args.multilabel else "softmax")
    n, ft = xs[0].shape
    print(f"nodes {n}, features {ft}, classes {nb_classes}, meta-paths {len(graphs)}, "
          f"edges {[g.nnz for g in graphs]}")

    model = HeteGAT_multi().build(len(graphs), ft, nb_classes, (8,), (8, 1), 128, device=dev, semantic=args.semantic)
    fanout = None
    if args.fanout is not None:
        if args.batch_size is None:
            ap.error("--fanout samples the blocks of --batch-size")
        try:
            fanout = [int(v) for v in args.fanout.split(",")]
        except ValueError:
            ap.error(f"--fanout {args.fanout}: expected F or F,F,...")
        fanout = fanout[0] if len(fanout) == 1 else fanout
    if args.batch_size is not None:
        if args.semantic == "metapath":
            ap.error("--batch-size: a block's mean score is not the graph's, --semantic metapath needs the whole graph")
        if args.graph:
            ap.error("--batch-size: the block shapes change per batch, there is no epoch to capture (--graph)")
        tr = MiniBatchTrainer(model, xs, graphs, labels, masks[0], masks[1], batch_size=args.batch_size, lr=0.005,
                              l2_coef=0.001, attn_drop=0.6, ffd_drop=0.6, seed=args.seed, patience=args.patience,
                              fanout=fanout, **objective)
        tr.overlap_eval = False
    else:
        tr = HANTrainer(model, xs, graphs, labels, masks[0], masks[1], lr=0.005, l2_coef=0.001,
                        attn_drop=0.6, ffd_drop=0.6, patience=args.patience, use_graph=args.graph,
                        overlap_eval=args.graph and args.overlap_eval, **objective)
    t0 = time.perf_counter()
    for epoch in range(args.epochs):
        tl, ta, vl, va = (float(v) for v in tr.epoch())
        if tr.overlap_eval and epoch == 0:
            continue                         # that pair belongs to the initial parameters (ex_acm3025.py has no such line)
        if epoch % 10 == 0:
            print(f"epoch {epoch:4d}  train loss {tl:.5f} {metric} {ta:.5f} | val loss {vl:.5f} {metric} {va:.5f}")
            if args.semantic == "metapath":      # the weights of the epoch's last forward (the validation one)
                print("            meta-path weights:", [round(v, 5) for v in model.metapath_weights.tolist()])
        if tr.early_stopping(vl, va):
            print(f"early stop at epoch {epoch}: min val loss {tr.vlss_mn:.5f}, max val {metric} {tr.vacc_mx:.5f}")
            break
    else:
        if tr.overlap_eval:                  # the validation pair of the last epoch
            tr.early_stopping(*(float(v) for v in tr.flush_eval()))
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(f"{epoch + 1} epochs in {dt:.2f} s ({(epoch + 1) / dt:.1f} epochs/s)")
    tr.restore_best()
    if args.batch_size is not None:
        tl, ta = tr.evaluate(masks[2])
    else:
        w_test = 1.0 / max(int(masks[2].sum()), 1)
        tl, ta = tr.eval_step(masks[2].to(torch.uint8).contiguous(), w_test)
    print(f"test loss {float(tl):.5f}  test {'micro-F1' if args.multilabel else 'accuracy'} {float(ta):.5f}")
    with torch.no_grad():
        _, final_embed, att = model.inference(xs, nb_classes, n, False, 0.0, 0.0, graphs, [8], [8, 1],
                                              semantic=args.semantic)
    print("mean meta-path attention:", att.mean(0).tolist())
    if args.eval_device == "gpu":
        sel = masks[2].bool()
        emb, lab, eval_dev = final_embed[sel], classes[sel], dev
    else:
        sel = masks[2].bool().cpu().numpy()
        emb, lab, eval_dev = final_embed.cpu().numpy()[sel], classes.cpu().numpy()[sel], None
    evaluate.my_KNN(emb, lab, seed=args.seed, device=eval_dev)                     # ex_acm3025.py:288
    evaluate.my_Kmeans(emb, lab, k=n_groups, seed=args.seed, device=eval_dev, silhouette=args.silhouette)    # :289
    if args.tsne:                                                                  # the picture of jhyexp.py:16
        import numpy as np
        coords, info = evaluate.tsne(emb, seed=args.seed, device=eval_dev, return_info=True)
        np.savez(args.tsne, coords=coords.cpu().numpy() if eval_dev is not None else coords,
                 labels=lab.cpu().numpy() if eval_dev is not None else lab)
        print(f"t-SNE: {info['n_iter']} iterations, KL divergence {info['kl_divergence']:.4f} -> {args.tsne}")


if __name__ == "__main__":
    main()
