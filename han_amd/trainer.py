"""Full-graph training loop of the reference (``ex_acm3025.py:171-245``) on the
HIP kernels: one epoch = ONE fwd+bwd+Adam step on the whole graph with dropout
0.6/0.6 on the train mask, then ONE eval forward on the val mask (both `while`
loops of the script run exactly once because batch_size = 1 = number of graphs).

`sess.run([train_op, loss, accuracy], feed_dict)` becomes :meth:`train_step`,
`sess.run([loss, accuracy], feed_dict)` becomes :meth:`eval_step`.  Under a
:class:`~han_amd.dist.NodePartition` every rank owns a block of rows; the only
collectives are the table all-gathers inside the node-attention op and one
all-reduce of the flat gradient buffer.
"""
from __future__ import annotations

import os

import torch

from . import layers, ops, rng
from .base_gattn import TFAdam
from .dist import NodePartition
from .features import SparseFeatures, as_features
from .gat import HeteGAT_multi
from .graph import as_graph


class _EvalBranch:
    """HANTrainer(overlap_eval=True): the eval forward of the parameters an epoch starts with, cut in the two pieces
    that fit the training step's fork / join sections: node_level() (K1 + K2 of every meta-path -> M) runs beside
    the training forward's per-meta-path chains, head() (K3, classifier, loss; the copy of the parameters) beside
    the backward's.  Each piece forks `stream` from the current stream, runs as one chain with scratch buffers of
    its own (ops.branch) and is joined by the section's own join (`join()`); with stream None the pieces run in
    place."""

    def __init__(self, trainer, stream):
        self.tr, self.stream = trainer, stream
        self.M = self.vl = self.va = None

    def _run(self, fn):
        m = self.tr.model
        streams, m.path_streams = m.path_streams, None        # one chain: K1 of every meta-path in one launch
        branch, m.overlap_branch = getattr(m, "overlap_branch", None), None
        try:
            if self.stream is not None:
                self.stream.wait_stream(torch.cuda.current_stream())
            with torch.no_grad(), ops.branch(self.stream, "@eval"):
                fn()
        finally:
            m.path_streams, m.overlap_branch = streams, branch

    def join(self):
        if self.stream is not None:
            torch.cuda.current_stream().wait_stream(self.stream)

    def node_level(self):
        tr = self.tr

        def fn():
            self.M = tr.model.node_level(tr.xs, tr.graphs, 0.0, 0.0, False, ops.ACT_ELU, graphs_t=tr.graphs_t)
        self._run(fn)

    def head(self):
        tr = self.tr

        def fn():
            Z, _ = tr.model.semantic(self.M)
            self.vl, self.va, _ = tr.model.classifier_loss(Z, tr.labels, tr.val_mask, tr.w_val)
            tr._flat_prev.copy_(tr.model.flat)
            self.M = None
        self._run(fn)


# HANTrainer(live_backward="auto") acts from this many rows on (the size from which side_stream="auto" acts).  The reason
# is compatibility, not a measurement: the live backward adds its terms in another order, and the default trainer on
# small graphs is what the existing parity tests pin to the bit (fold on against off, the fused entry's lower row bound,
# the zero-rows hint on every gather).  live_backward=True has no such floor.
LIVE_BACKWARD_MIN_ROWS = 262144


# HANTrainer(live_forward="auto") acts from this many rows on.  A constant of its own, so that patching the backward's
# does not switch the forward on: below it the default trainer keeps the launches (and the whole-graph M, Z and logits)
# that the small-graph tests look at.  live_forward=True has no such floor.
LIVE_FORWARD_MIN_ROWS = 262144


OBJECTIVES = ("softmax", "sigmoid")


def check_objective(objective, labels, n_classes: int, partitioned: bool = False):
    """The constructor checks of HANTrainer / MiniBatchTrainer(objective=...); host-side, before anything is built."""
    if objective not in OBJECTIVES:
        raise ValueError(f"objective = {objective!r}: expected one of {OBJECTIVES}")
    if objective != "sigmoid":
        return
    if partitioned:
        raise NotImplementedError("objective='sigmoid' under a node partition is not supported: micro-F1 is not a sum "
                                  "over ranks (its counts tp / fp / fn are, and are not exchanged yet)")
    if labels.dim() != 2 or labels.shape[1] != n_classes:
        raise ValueError(f"objective='sigmoid': labels must be an (N, {n_classes}) multi-hot matrix, got "
                         f"{tuple(labels.shape)}")


def metric_improved(value: float, best: float) -> bool:
    """value >= best for the early-stopping rule of both trainers; a NaN value never is."""
    return value == value and value >= best


def device_labels(objective, labels, dev):
    """The label tensor the classifier kernels read: (N,) int32 class ids, or the packed words of a multi-hot matrix."""
    if objective == "sigmoid":
        return ops.pack_label_bits(labels.to(dev)).contiguous()
    return labels.to(device=dev, dtype=torch.int32).contiguous()


class HANTrainer:
    def __init__(self, model: HeteGAT_multi, xs, graphs, labels, train_mask, val_mask=None,
                 lr=0.005, l2_coef=0.001, attn_drop=0.6, ffd_drop=0.6,
                 part: NodePartition | None = None, patience=100, max_halo_fraction=0.6,
                 use_graph=False, graphs_local=False, xs_full=None, replicate="auto", masked_backward=False,
                 side_stream=False, overlap_eval=False, live_backward="auto", live_forward="auto",
                 shared_projection="auto", objective="softmax"):
        """objective ("softmax" | "sigmoid"): "softmax" is the single-label step (labels (N,) class ids; the second
        scalar of train_step / eval_step / epoch is the masked accuracy).  "sigmoid" is the reference's multi-label
        pair, models/base_gattn.py:50-59,71-94: labels is an (N, C) multi-hot matrix, packed once
        (ops.pack_label_bits), the loss is the masked sigmoid cross-entropy and the second scalar is micro-F1, on which
        early_stopping, checkpoints and resume then work as they do on the accuracy (NaN -- no true positive yet --
        never counts as an improvement).  Everything below or beside the classifier (live_forward, live_backward,
        fold_k3, the captured epoch, overlap_eval) is unchanged.  Not under a node partition: micro-F1 is not a sum
        over ranks (its counts are; exchanging them is left open), so that raises here.
        xs: list of P (N_local,F) feature tensors (this rank's rows), or sparse features (SparseFeatures / torch
        sparse COO or CSR tensors; single process only);
        graphs: list of P CSRGraph (or dense masks / CSR tuples).  Under a partition (`part`) either
        the GLOBAL graphs (graphs_local=False: each rank keeps its row block; small data sets) or --
        graphs_local=True, the scalable form -- THIS RANK'S destination rows [row_start, row_end) with
        global column ids, so that no rank ever holds a global graph; the transposed shards are then
        built with an all-to-all-v of the edges (NodePartition.shard_local_graph);
        labels int32 (N_local,) class ids; masks uint8/bool (N_local,).
        side_stream: False | True | "auto" -- the eager training step of a single process runs the backward's dW of
        meta-path p on a second stream beside the transposed-graph gather of meta-path p + 1 (layers.NodeLevelAttention.backward): +1.3-2.5 %
        epochs/s at SYN-1M, bit-equal results.  Off by default: the gather's launch time then includes that company and
        no longer measures the gather.  "auto" = on from 262 144 table rows, where a gather is long enough to hide a dW.
        use_graph: capture one whole epoch (train step + eval forward, ~60 launches) into a
        hipGraph on its second call and replay it afterwards -- for the launch-bound small
        graphs (ACM / DBLP sizes).  The per-step dropout seed and Adam's step count then live
        in a 2-word device state that the graph itself advances (han_hip.h "Seeds").
        Single-process only.
        overlap_eval (with use_graph; False | True = "branch" | "sections"): the eval forward needs the parameters one
        training step produced and nothing else of it, and the next step's forward and backward only READ those
        parameters -- so the captured epoch runs
        the eval forward of the parameters it STARTS with as a second branch of the graph beside its own training
        forward and backward, and only Adam waits for both.  Every number is the one the plain epoch computes, the
        validation pair arrives one call later: call k returns (train loss / accuracy of step k, validation loss /
        accuracy of the parameters BEFORE step k, i.e. of epoch k - 1; the first call evaluates the initial
        parameters).  `flush_eval()` evaluates the current parameters (the validation pair of the last epoch), and
        `early_stopping` snapshots the parameters the validation pair belongs to.  For the launch-bound small
        graphs, where the eval chain (about a fifth of the epoch's dependent launches) then hides under the
        training step; on graphs that fill the machine it buys nothing.  "branch": ONE branch from the epoch's first
        node to Adam (one box, 400 replays: ACM-like 0.394 -> 0.325 ms per epoch, DBLP-like 0.859 -> 0.828 with the
        per-meta-path chains issued largest graph first, layers._path_order); "sections": the eval forward in two
        pieces inside the training step's own fork / join sections -- K1 + K2 beside the training forward's
        per-meta-path chains, K3 + classifier beside the backward's (ACM-like 0.384, DBLP-like 0.858 on another box
        whose plain epochs took 0.398 / 0.891).
        xs_full: under a partition, optionally the features of ALL rows (P tensors (N,F), the same on
        every rank): the forward passes named by `replicate` ("auto" = dist.replication_policy,
        "all", "eval", "none") then project the whole table on every rank instead of exchanging it;
        `xs` may then be None (the local rows are views of xs_full).
        The trainer sets model.direct_grads(True) and model.fold_k3 = True and leaves them set: both describe ITS step
        (every parameter used once, M consumed by semantic() alone).  A model used free-form afterwards with another
        consumer of M raises in the backward (layers.FoldTail); set model.fold_k3 = False for that.
        live_forward ("auto" | True | False): epoch() returns four scalars -- the training loss and accuracy, sums over
        the train mask, and the validation pair, a sum over the val mask -- and with one node-attention layer and a
        row-local K3 and classifier, row i of M, Z and the logits influences them only when i is in the mask.  The
        reference's sess.run([train_op, loss, accuracy]) (ex_acm3025.py:190) fetches the same scalars; TensorFlow
        computes every row there only because its dense ops cannot do otherwise.  So K1 still projects every row (H is
        the gather table), and the K2 gather, K3 and the classifier run over the masked rows only
        (layers.LiveForwardPlan, one per mask, shared when both masks are one tensor), and so does K3.  A
        listed row gets the bits the full forward gives it; the sums over the rows are taken in another order.  The eval
        forward does so where all of these hold -- CUDA, one node-attention layer of the 8 x 8 head shape, at most 64
        classes, no node partition, a mask of at most half of the rows -- and, for "auto", the graphs have at least
        LIVE_FORWARD_MIN_ROWS rows; eval_step(mask=other) with any other mask runs the full forward.  The training
        forward does so ONLY in a step whose backward is the row-list fold of live_backward (fp32 tables, no residual,
        no per-meta-path streams, masked backward off, a K3 of han_sem_attn_bwd_rows_live's shapes): every other
        backward reads M and aggp of every row.  True: ValueError where the eval conditions fail.  Whole-graph
        embeddings and logits remain what inference / predict return: those paths are not touched.
        live_backward ("auto" | True | False): the backward computes exactly the terms that are not identically zero.  With a single
        node-attention layer, a row-local K3 and classifier and a train mask that never changes, dZ_i, dM_i and g_i are
        exactly zero for every row i outside the mask, so the set-up builds, once, the list of live rows and per
        meta-path the transposed graph with only the entries whose destination is live (layers.LiveBackwardPlan); the
        K3 backward then runs over the list and the gather over that graph.  Same terms, another summation order
        (per-lane order of dH / df2, tile grouping of dw / db / du / dc): results agree to rounding, not to the bit.
        "auto": on where all of these hold -- CUDA, no further node-attention layer, at most half of the rows in the
        train mask, no node partition, masked_backward off -- and the graphs have at least LIVE_BACKWARD_MIN_ROWS rows
        (below that the default keeps the bits of the full backward, which the small-graph parity tests pin; the gain
        there has not been measured); True: on at any size (ValueError where one of the other conditions fails, masked_backward
        still wins); False: every row in the backward too.
        shared_projection ("auto" | True | False): inside epoch() the eval forward projects X with the parameters the next
        training forward projects it with again, under dropout.  Its K1 then runs as ops.project_fwd_both -- one pass
        over X per meta-path that gives the eval tables and, under the next step's seeds (rng.peek_seeds), the
        training tables -- and the next training forward takes those in place of its own K1 (layers.SharedProjection:
        only when seeds, dropout rates, features and parameters are what it would use itself; every public path that
        writes parameters drops them).  Byte for byte the same tables, so the same epochs.  A bare eval_step() is
        not touched.  The waiting tables hold P x (N x 64 x 4 + 2 x N x 8 x 4 + N x F) bytes: 4 x (256 + 64 + 256) MB
        at N = 1M, P = 4, F = 256.  It acts where all of these hold: CUDA, one node-attention layer of 8 x 8 heads on
        fp32 tables, ONE dense fp32 feature tensor with finite values for every meta-path, an even number of them,
        at least 32 768 rows (the row count from which K1 writes a keep table), input dropout, no node partition, no
        captured epoch.  "auto" also declines when the waiting tables would take more than a quarter of the device
        memory that is free at construction; True raises ValueError where it cannot act; False is the two separate
        calls.
        masked_backward: OPT-IN (never the default, never the headline measurement): the transposed-graph pass keeps
        the dead entries in place and skips them one by one (bit-identical results, dist.MaskedBackwardPlan)
        and, under a partition, only the live rows of the backward table travel.  Switches live_backward off.
        A model built with semantic="metapath" (one weight per meta-path, han.pdf eq. 7-9) is not row-local: live_forward
        and live_backward "auto" resolve to off and True raises ValueError, masked_backward=True raises ValueError, a
        node partition raises NotImplementedError, fold_k3 has no effect; shared_projection, side_stream, use_graph and
        overlap_eval work as in the node mode."""
        if not model._built:
            raise RuntimeError("build the model first (model.build(...))")
        self.objective = objective
        check_objective(objective, labels, model.Wc.shape[2], part is not None and part.active)
        self.model = model
        model.direct_grads(True)      # gradients land in model.flat_grad without copy/accumulate launches
        model.fold_k3 = True          # M goes from node_level() straight into semantic(): the K3 backward runs the row-local K2 backward too
        self.part = part if (part is not None and part.active) else None
        # semantic="metapath" (han.pdf eq. 7-9): the mean of a meta-path's scores runs over EVERY node and dM has no zero
        # rows, so nothing that relies on row-locality applies -- "auto" resolves to off, an explicit request raises
        metapath = model.semantic_mode == "metapath"
        if metapath:
            why = ('semantic="metapath": the weight of a meta-path is the mean of its scores over every node, and every '
                   "row of dM depends on every row of dZ; ")
            if self.part is not None:
                raise NotImplementedError(why + "under a node partition the mean is a sum over ranks (two all-reduces of "
                                          "P doubles per step), which is not built")
            if live_forward is True or live_backward is True:
                raise ValueError(why + "live_forward / live_backward visit only the rows of a mask")
            if masked_backward:
                raise ValueError(why + "masked_backward drops the rows outside the train mask")
            live_forward = False if live_forward == "auto" else live_forward
            live_backward = False if live_backward == "auto" else live_backward
        layers._no_sparse_under_partition(self.part is not None or xs_full is not None, xs, xs_full)
        model.partition = self.part
        dev = model.flat.device
        self.xs_full, self.replicate, self.replicate_info = None, frozenset(), None
        self._replicate_arg = replicate
        if xs_full is not None and self.part is not None:
            from .dist import replication_policy
            pt = self.part
            if any(x.shape[0] != pt.n_global for x in xs_full):
                raise ValueError("xs_full must hold the features of all %d rows" % pt.n_global)
            if xs is None:
                xs = [x[pt.row_start:pt.row_end] for x in xs_full]
            # the exchanged tables have world * shard rows (the last shard may be short): pad once
            pad = {}
            for x in xs_full:      # the P meta-paths usually share one feature tensor
                if id(x) not in pad:
                    xc = x.contiguous()
                    if pt.n_table != pt.n_global:
                        xc = torch.cat([xc, xc.new_zeros((pt.n_table - pt.n_global, xc.shape[1]))])
                    pad[id(x)] = xc
            self.xs_full = tuple(pad[id(x)] for x in xs_full)
            self.replicate = replication_policy(pt.world, replicate)
            self.replicate_info = {"policy": "static (han_amd.dist.replication_policy)"}
        self.xs = [x if isinstance(x, SparseFeatures) else x.contiguous() for x in map(as_features, xs)]
        graphs = [as_graph(g, dev) for g in graphs]     # dense masks / (rowptr, colidx) accepted
        if self.part is not None:
            sharded = [self.part.shard_local_graph(g) if graphs_local else self.part.shard_graph(g)
                       for g in graphs]
            self.graphs = [s[0] for s in sharded]
            self.graphs_t = [s[1] for s in sharded]
            # halo exchange where the graph has locality, all-gather where it has none
            model.halo_plans = ([self.part.plan_exchange(g, max_halo_fraction) for g in self.graphs],
                                [self.part.plan_exchange(g, max_halo_fraction) for g in self.graphs_t])
        else:
            self.graphs = list(graphs)
            self.graphs_t = [g.transpose() for g in graphs]
            model.halo_plans = (None, None)
        if self.xs_full is not None and self._replicate_arg == "auto" and "HAN_REPLICATE" not in os.environ:
            self._calibrate_replication(ffd_drop)
        self.labels = device_labels(objective, labels, dev)
        self.train_mask = train_mask.to(device=dev, dtype=torch.uint8).contiguous()
        self._masked_plans = None
        if live_backward not in ("auto", True, False):
            raise ValueError(f"live_backward = {live_backward!r}: expected 'auto', True or False")
        self._live_plan = None
        self._live_fwd_train = None
        n_all = self._global_count(torch.ones_like(self.train_mask))
        live_ok = (dev.type == "cuda" and not model.extra and self.part is None
                   and 2 * self._global_count(self.train_mask) <= n_all)
        if live_backward is True and not live_ok:
            raise ValueError("live_backward=True needs a CUDA model with one node-attention layer, no node partition and "
                             "a train mask of at most half of the rows")
        if live_ok and (live_backward is True or (live_backward == "auto" and n_all >= LIVE_BACKWARD_MIN_ROWS)):
            self._live_plan = layers.LiveBackwardPlan(self.graphs_t, self.train_mask)
        self.set_masked_backward(masked_backward)
        # one tensor for both masks when the caller gave one: the plans below are looked up by the mask tensor's identity
        # and built from its values once -- the masks are constructor arguments and must not be edited in place afterwards
        # (an edit of the one would also be an edit of the other, and the row lists would go stale)
        same_masks = val_mask is None or val_mask is train_mask
        self.val_mask = self.train_mask if same_masks else val_mask.to(device=dev, dtype=torch.uint8).contiguous()
        if live_forward not in ("auto", True, False):
            raise ValueError(f"live_forward = {live_forward!r}: expected 'auto', True or False")
        self._live_fwd = {}      # id(mask tensor) -> (mask, layers.LiveForwardPlan): train mask, val mask
        shape_ok = (dev.type == "cuda" and not model.extra and self.part is None and model.K == 8 and model.FP == 8
                    and model.Wc.shape[2] <= layers.MAX_CLASSES)

        def fwd_ok(mask):
            return shape_ok and 2 * self._global_count(mask) <= n_all
        if live_forward is True and not fwd_ok(self.val_mask):
            raise ValueError("live_forward=True needs a CUDA model with one node-attention layer of 8 x 8 heads, at most "
                             "64 classes, no node partition and a val mask of at most half of the rows")
        if live_forward is True or (live_forward == "auto" and n_all >= LIVE_FORWARD_MIN_ROWS):
            if fwd_ok(self.val_mask):
                self._live_fwd[id(self.val_mask)] = (self.val_mask, layers.LiveForwardPlan(self.graphs, self.val_mask))
            # the training forward: only beside the row-list fold, whose K3 shapes are han_sem_attn_bwd_rows_live's
            A, P = model.w_omega.shape[1], len(self.graphs)
            if (self._live_plan is not None and shape_ok and A in (64, 128) and P in (1, 2, 4)
                    and tuple(model.w_omega.shape) == (ops.D, A) and n_all * ops.gs_row_bytes() < (1 << 32)):
                mine = self._live_fwd.get(id(self.train_mask))
                plan = layers.LiveForwardPlan(self.graphs, self.train_mask, backward=self._live_plan)
                if mine is not None:      # one mask for both: one plan, one set of row lists
                    plan._subsets = mine[1]._subsets
                self._live_fwd_train = plan

        if shared_projection not in ("auto", True, False):
            raise ValueError(f"shared_projection = {shared_projection!r}: expected 'auto', True or False")
        model.shared_proj = None
        x0 = self.xs[0] if self.xs else None
        P_ = len(self.graphs)
        share_ok = (dev.type == "cuda" and not model.extra and self.part is None and not use_graph and not overlap_eval
                    and model.K == 8 and model.FP == 8 and model.table_dtype == torch.float32 and P_ >= 2 and P_ % 2 == 0
                    and float(ffd_drop) > 0 and isinstance(x0, torch.Tensor) and x0.dtype == torch.float32
                    and all(x is x0 for x in self.xs)
                    and ops.keep_bytes(x0.shape[0], x0.shape[1], x0.stride(0), 8, 8) > 0
                    and bool(torch.isfinite(x0).all()))      # (the combined kernel's one condition on the VALUES: han_hip.h)
        if shared_projection is True and not share_ok:
            raise ValueError("shared_projection=True needs a CUDA model with one node-attention layer of 8 x 8 heads and fp32 "
                             "tables, one dense fp32 feature tensor of at least 32 768 rows shared by an even number of "
                             "meta-paths, input dropout, no node partition, no captured epoch and no overlap_eval")
        if share_ok and shared_projection == "auto":
            need = layers.SharedProjection.stash_bytes(x0.shape[0], x0.shape[1], P_)
            share_ok = 4 * need <= torch.cuda.mem_get_info(dev)[0]
        if share_ok and shared_projection is not False:
            model.shared_proj = layers.SharedProjection(lambda: model.flat, lambda: self.opt.t)

        # mean(loss * mask / mean(mask)) == sum(mask * loss) / count(mask): the
        # normaliser is a setup-time constant, summed over ranks once.
        self.w_train = 1.0 / max(self._global_count(self.train_mask), 1)
        self.w_val = 1.0 / max(self._global_count(self.val_mask), 1)
        # a hint, not a plan: with one node-attention layer the g row of a destination outside the mask is zero, and the
        # HIP backward gather skips what its producers flag as zero (HAN_FLAG_K2_ZERO_ROWS) -- a gain from half of the
        # rows on, a small loss where every row is live.  Single GPU only in effect: under a node
        # partition the backward tables come with an id table, those launches are not predicated and ignore the hint.
        n_global = self._global_count(torch.ones_like(self.train_mask))
        model.zero_rows = dev.type == "cuda" and not model.extra and 2 * self._global_count(self.train_mask) <= n_global
        self.opt = TFAdam(model.flat, model.flat_grad, lr=lr, l2_coef=l2_coef)
        # d loss = 1 handed to backward() instead of the ones_like() autograd would launch per step: in a captured epoch
        # of the small graphs that 1-element fill is a dependent 5-us launch between the loss and the K3 backward
        self._one = torch.ones((), dtype=torch.float32, device=dev)
        self.attn_drop, self.ffd_drop = attn_drop, ffd_drop
        self.patience = patience
        self.vlss_mn, self.vacc_mx, self.curr_step = float("inf"), 0.0, 0
        self.best_state = None
        self.use_graph = bool(use_graph)
        if overlap_eval not in (False, True, "branch", "sections"):
            raise ValueError(f"overlap_eval = {overlap_eval!r}: expected False, True, 'branch' or 'sections'")
        self.overlap_eval = bool(overlap_eval)
        self.overlap_form = "sections" if overlap_eval == "sections" else "branch"
        if self.overlap_eval and not self.use_graph:
            raise ValueError("overlap_eval reorders the captured epoch: it needs use_graph=True")
        self._eval_stream = None
        self._force_segments = False  # tests: run the two-piece flow of the captured epoch in place (any backend)
        self._flat_prev = None        # overlap_eval: the parameters the returned validation pair was computed with
        self._capture = True          # tests switch this off to run the same device-state flow eagerly
        self._graph = None
        self._static_out = None
        self._graph_calls = 0
        n_rows = int(self.graphs[0].n_rows) if len(self.graphs) else 0
        want_side = (n_rows >= 262144) if side_stream == "auto" else bool(side_stream)
        if want_side and not self.use_graph and self.part is None and dev.type == "cuda" and len(self.graphs) > 1:
            model.side_stream = torch.cuda.Stream(device=dev)
        if self.use_graph:
            if self.part is not None:
                raise NotImplementedError("use_graph is for single-process training")
            # [seed word, Adam step count]; advanced by the first op of every epoch
            self.step_state = torch.zeros(2, dtype=torch.int64, device=dev)
            self.step_state[1] = self.opt.t
            self._step_inc = torch.tensor([-0x61C8864680B583EB, 1], dtype=torch.int64, device=dev)  # 0x9E37...15
            model.step_seed_dev = self.step_state[0:1]
            self.opt.step_dev = self.step_state[1:2]
            # one stream per meta-path: inside the captured epoch the per-meta-path chains (K1 -> K2, and the four
            # backward kernels) become parallel branches of the graph -- at these sizes every kernel is a few
            # microseconds on a few CUs (layers._each_path); HAN_PATH_STREAMS=0 keeps the single chain
            if dev.type == "cuda" and os.environ.get("HAN_PATH_STREAMS", "1") != "0" and len(self.graphs) > 1:
                model.path_streams = [torch.cuda.Stream(device=dev) for _ in self.graphs]
            if self.overlap_eval:
                model.path_order = "heavy"
                self._flat_prev = torch.empty_like(model.flat)
                if dev.type == "cuda":
                    self._eval_stream = torch.cuda.Stream(device=dev)

    @property
    def live_backward(self) -> bool:
        """Whether the backward runs over the live rows only (the live_backward argument, as decided)."""
        return self.model.live_bwd is not None

    @property
    def shared_projection(self) -> bool:
        """Whether epoch()'s eval forward also projects for the next training forward (the shared_projection argument, as decided)."""
        return self.model.shared_proj is not None

    def _drop_shared(self):
        if self.model.shared_proj is not None:
            self.model.shared_proj.drop()

    @property
    def live_forward(self) -> bool:
        """Whether the eval forward of the val mask runs over its rows only (the live_forward argument, as decided)."""
        return id(self.val_mask) in self._live_fwd

    def set_masked_backward(self, flag: bool):
        """Switch the opt-in masked backward on or off (plans are built on first use; collective under a partition)."""
        if flag and self.model.semantic_mode == "metapath":
            raise ValueError('semantic="metapath": every row of dM depends on every row of dZ; masked_backward drops the '
                             "rows outside the train mask")
        self.masked_backward = bool(flag)
        self.model.live_bwd = None if self.masked_backward else self._live_plan      # the masked backward wins
        if not self.masked_backward:
            self.model.masked_bwd = None
            return
        if getattr(self, "use_graph", False) and self._graph is not None:
            raise RuntimeError("the epoch is already captured; choose masked_backward before the first epoch")
        if self.model.extra:
            raise NotImplementedError("masked_backward needs a single node-attention layer: with more, the rows "
                                      "outside the mask feed the rows inside it")
        if self._masked_plans is None:
            from .dist import MaskedBackwardPlan
            live_global = self.part.all_gather_rows(self.train_mask) if self.part is not None else None
            self._masked_plans = [MaskedBackwardPlan(self.part, gt, self.train_mask, live_global)
                                  for gt in self.graphs_t]
        self.model.masked_bwd = self._masked_plans

    def _calibrate_replication(self, ffd_drop, reps=3):
        """replicate="auto" over RCCL: MEASURE, on this machine and this shape, what a forward table costs to
        exchange (one all-gather of a rank's projected rows) against what it costs to recompute (K1 over all
        rows minus K1 over the local rows, with and without dropout), take the maximum over the ranks and
        replicate exactly the forward passes whose projection is cheaper than their exchange.  Other
        backends (the gloo rehearsals, whose timings mean nothing) keep the static policy."""
        import torch.distributed as dist
        pt = self.part
        if not (dist.is_available() and dist.is_initialized() and dist.get_backend(pt.group) == "nccl"):
            return
        if all(pl is not None for pl in self.model.halo_plans[0]):
            return                                  # every meta-path has a halo plan: nothing to decide
        m, dev = self.model, self.model.flat.device
        Xf, Xl = self.xs_full[0], self.xs[0]
        F = Xf.shape[1]
        W = torch.zeros((F, ops.D), device=dev)     # K1's time does not depend on the values
        a, b = torch.zeros((8, 8), device=dev), torch.zeros(8, device=dev)

        def ms(fn):
            fn()
            torch.cuda.synchronize()
            ts = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                ts.append(e0.elapsed_time(e1))
            return sorted(ts)[len(ts) // 2]

        def k1(X, drop, off):
            return ops.project_fwd(X, W, a, a, b, b, in_drop=drop, fts_drop=drop, seed=1, row_offset=off,
                                   table_dtype=m.table_dtype)

        with torch.no_grad():
            t = [ms(lambda: k1(Xl, ffd_drop, pt.row_start)), ms(lambda: k1(Xf, ffd_drop, 0)),
                 ms(lambda: k1(Xl, 0.0, pt.row_start)), ms(lambda: k1(Xf, 0.0, 0))]
            H_loc = k1(Xl, 0.0, pt.row_start)[0]
            t.append(ms(lambda: pt.all_gather_rows_async(H_loc, ("calib",)).wait()))
        tt = torch.tensor(t, device=dev, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX, group=pt.group)
        loc_tr, full_tr, loc_ev, full_ev, gather = (float(v) for v in tt.tolist())
        rep = set()
        if full_tr - loc_tr < gather:
            rep.add("train")
        if full_ev - loc_ev < gather:
            rep.add("eval")
        self.replicate = frozenset(rep)
        self.replicate_info = {"policy": "measured at set-up (max over ranks, ms)",
                               "all_gather_of_one_forward_table": round(gather, 3),
                               "extra_projection_training": round(full_tr - loc_tr, 3),
                               "extra_projection_eval": round(full_ev - loc_ev, 3)}
        pt.drop_buffers(("calib",))

    def _global_count(self, mask):
        c = mask.sum().to(torch.float32).reshape(1)
        if self.part is not None:
            self.part.all_reduce_sum_(c)
        return int(c.item())

    def _forward(self, train: bool, mask, weight):
        m = self.model
        if train:      # the train mask; NodeLevelAttention.forward declines where the backward is not the row-list fold
            plan = self._live_fwd_train
        else:          # the mask the plan was built for, and no other
            plan = self._live_fwd.get(id(mask), (None, None))
            plan = plan[1] if plan[0] is mask else None
        with torch.set_grad_enabled(train):
            M = m.node_level(self.xs, self.graphs, self.attn_drop if train else 0.0,
                             self.ffd_drop if train else 0.0, train, ops.ACT_ELU,
                             graphs_t=self.graphs_t,
                             xs_full=self.xs_full if ("train" if train else "eval") in self.replicate else None,
                             live_fwd=plan)
            Z, _ = m.semantic(M)
            loss, acc, _ = m.classifier_loss(Z, self.labels, mask, weight)
        return loss, acc

    def train_step(self):
        """sess.run([train_op, loss, accuracy]) with drop = 0.6 (ex_acm3025.py:178-193).
        Returns device scalars (this rank's share of) loss and accuracy."""
        self.model.zero_grad_flat()
        loss, acc = self._forward(True, self.train_mask, self.w_train)
        loss.backward(self._one)
        if self.part is not None:
            self.part.all_reduce_sum_(self.model.flat_grad)
        self.opt.step()
        return loss.detach(), acc

    def eval_step(self, mask=None, weight=None):
        """sess.run([loss, accuracy]) with drop = 0.0 (ex_acm3025.py:199-218)."""
        mask = self.val_mask if mask is None else mask
        weight = self.w_val if weight is None else weight
        loss, acc = self._forward(False, mask, weight)
        return loss, acc

    def epoch(self):
        """One reference epoch; returns device tensors (no host sync).  With use_graph the
        tensors are the graph's static outputs: the next epoch() overwrites them."""
        if self.use_graph:
            return self._epoch_graph()
        tl, ta = self.train_step()
        sp = self.model.shared_proj
        if sp is None:
            vl, va = self.eval_step()
            return tl, ta, vl, va
        sp.armed = float(self.ffd_drop)      # this eval forward's K1 also projects for the next training forward
        try:
            vl, va = self.eval_step()
        finally:
            sp.armed = None
        return tl, ta, vl, va

    def _epoch_body(self):
        self.step_state.add_(self._step_inc)
        if self.overlap_eval:
            return self._epoch_body_overlapped()
        tl, ta = self.train_step()
        vl, va = self.eval_step()
        return tl, ta, vl, va

    def _eval_branch(self):
        """The eval forward of the CURRENT parameters as ONE chain (launched eagerly: the warm-up epoch, the tests'
        eager flow, the CPU stand-in backend), and the copy of those parameters that early_stopping checkpoints."""
        br = _EvalBranch(self, None)
        br.node_level()
        br.head()
        return br.vl, br.va

    def _epoch_body_overlapped(self):
        if not self._force_segments and (self._eval_stream is None or not torch.cuda.is_current_stream_capturing()):
            # launched eagerly (the warm-up epoch, which also BUILDS the graphs' cached row lists and transposes on the
            # stream it runs on): one chain, same order of values
            vl, va = self._eval_branch()
            tl, ta = self.train_step()
            return tl, ta, vl, va
        if self.overlap_form == "branch" and not self._force_segments:
            # one branch from the epoch's first node to Adam, beside the whole training forward and backward
            br = _EvalBranch(self, self._eval_stream)
            br.node_level()
            br.head()
            self.model.zero_grad_flat()
            loss, acc = self._forward(True, self.train_mask, self.w_train)
            loss.backward(self._one)
            br.join()                                         # Adam overwrites what the branch reads
            self.opt.step()
            return loss.detach(), acc, br.vl, br.va
        # "sections": the eval forward rides in the training step's own fork / join sections (layers.NodeLevelAttention:
        # K1 + K2 of all meta-paths beside the training forward's per-meta-path chains, K3 + classifier beside the
        # backward's) -- a series-parallel graph like the plain epoch's
        br = _EvalBranch(self, None if self._force_segments else self._eval_stream)
        m = self.model
        m.overlap_branch = br
        try:
            tl, ta = self.train_step()
        finally:
            m.overlap_branch = None
        if br.vl is None:
            raise NotImplementedError("overlap_eval: the first node-attention layer did not run through "
                                      "layers.NodeLevelAttention (head shapes beyond 8 x 8 columns)")
        return tl, ta, br.vl, br.va

    def flush_eval(self):
        """overlap_eval: the validation pair of the CURRENT parameters (the one the next epoch() would return),
        launched eagerly; a no-op alias of eval_step() otherwise."""
        if self.overlap_eval and self._flat_prev is not None:
            vl, va = self.eval_step()
            self._flat_prev.copy_(self.model.flat)
            return vl, va
        return self.eval_step()

    def _epoch_graph(self):
        self._graph_calls += 1
        if self._graph is not None:
            self.opt.t += 1                      # the replayed han_adam_step reads the device count
            self._graph.replay()
            return self._static_out
        if self._graph_calls == 1 or not self._capture or not self.model.flat.is_cuda:
            # warm-up epoch (a real one) on a side stream: sizes every workspace, builds the
            # cached transposes / row splits, lets autograd set up its buffers
            if not self.model.flat.is_cuda:
                return self._epoch_body()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                out = self._epoch_body()
            torch.cuda.current_stream().wait_stream(side)
            return out
        from . import _lib
        g = torch.cuda.CUDAGraph()
        calls0 = _lib.CALLS
        with torch.cuda.graph(g):
            self._static_out = self._epoch_body()   # recorded, not run (opt.t advanced by step())
        self.graph_abi_calls = _lib.CALLS - calls0   # C-ABI calls recorded into the epoch (each is 1-3 kernel nodes)
        self._graph = g
        g.replay()
        return self._static_out

    def reduce_metrics(self, *vals):
        """Sum per-rank partial losses/accuracies (they are already weighted by
        the global mask count) -- logging only, not needed for training."""
        t = torch.stack([v.reshape(()) for v in vals])
        if self.part is not None:
            self.part.all_reduce_sum_(t)
        return [float(x) for x in t.tolist()]

    def early_stopping(self, val_loss: float, val_acc: float) -> bool:
        """ex_acm3025.py:225-240: checkpoint when val acc >= best AND val loss <= best;
        stop after `patience` epochs without either improving.  Returns True to stop.
        A NaN metric (micro-F1 of objective="sigmoid" while nothing is predicted correctly: tp == 0) is no improvement
        and is never stored: max(nan, x) is nan, and every later comparison against a stored nan would be False."""
        acc_ok = metric_improved(val_acc, self.vacc_mx)
        if acc_ok or val_loss <= self.vlss_mn:
            if acc_ok and val_loss <= self.vlss_mn:
                # overlap_eval: the pair belongs to the parameters before the step that ran beside it
                src = self._flat_prev if self.overlap_eval else self.model.flat
                self.best_state = src.detach().clone()
            self.vacc_mx = max(val_acc, self.vacc_mx) if acc_ok else self.vacc_mx
            self.vlss_mn = min(val_loss, self.vlss_mn)
            self.curr_step = 0
            return False
        self.curr_step += 1
        return self.curr_step == self.patience

    def _signature(self):
        m = self.model
        sig = {"param_shapes": [(n, list(s)) for n, s in m.param_shapes()], "residual": bool(m.residual),
               "table_dtype": str(m.table_dtype), "use_graph": self.use_graph}
        if m.semantic_mode != "node":      # a "node" signature is as it always was: earlier checkpoints still load
            sig["semantic"] = m.semantic_mode
        return sig

    def save_checkpoint(self, path):
        """saver.save(sess, checkpt_file) (ex_acm3025.py:229) -- plus what the reference does not keep
        and a bit-exact resume needs: the optimiser state, the dropout seed stream (host counter, or the
        device step word of a captured epoch), and the early-stopping bookkeeping incl. the best weights."""
        ck = {"flat": self.model.flat.detach().cpu(),
              "opt": {"t": self.opt.t, "m": self.opt.m.cpu(), "v": self.opt.v.cpu()},
              "signature": self._signature(),
              "rng": dict(rng._state),
              "fixed_seeds": {f"{k[0]}:{k[1]}": list(v) for k, v in self.model._fixed_seeds.items()},
              "step_state": self.step_state.cpu() if self.use_graph else None,
              "early_stop": {"vlss_mn": self.vlss_mn, "vacc_mx": self.vacc_mx, "curr_step": self.curr_step},
              "best_state": self.best_state.cpu() if self.best_state is not None else None}
        torch.save(ck, path)

    def load_checkpoint(self, path):
        ck = torch.load(path, weights_only=True)
        sig = self._signature()
        if ck.get("signature") != sig:
            raise ValueError("checkpoint was written for a different model / trainer configuration: "
                             f"{ck.get('signature')} vs {sig}")
        m = self.model
        self._drop_shared()
        m.flat.copy_(ck["flat"])
        self.opt.load_state_dict(ck["opt"])
        rng._state.update(ck["rng"])
        fixed = {(int(k.split(":")[0]), int(k.split(":")[1])): tuple(v) for k, v in ck["fixed_seeds"].items()}
        if self._graph is not None and fixed != m._fixed_seeds:
            raise RuntimeError("this trainer has already captured its epoch with other per-meta-path seed "
                               "constants baked in; load the checkpoint before the first epoch")
        m._fixed_seeds = fixed
        if self.use_graph:
            self.step_state.copy_(ck["step_state"])
            self.step_state[1] = self.opt.t
        es = ck["early_stop"]
        self.vlss_mn, self.vacc_mx, self.curr_step = float(es["vlss_mn"]), float(es["vacc_mx"]), int(es["curr_step"])
        self.best_state = ck["best_state"].to(m.flat.device) if ck["best_state"] is not None else None

    def restore_best(self):
        """saver.restore(sess, checkpt_file) (ex_acm3025.py:247)."""
        if self.best_state is not None:
            self._drop_shared()
            self.model.flat.copy_(self.best_state)
