"""Ego blocks: mini-batch inference and training on the neighbourhood of a batch of seed nodes.

The reference's loop is a batch loop that runs once (``ex_acm3025.py:176-191``, ``batch_size = 1`` graph): the model
only ever sees the whole graph.  :func:`ego_block` cuts out of the P meta-path graphs the block a batch needs -- the
seeds and every node within ``hops`` steps of one over the UNION of the graphs -- with the nodes renumbered in
ascending order.  A node closer than ``hops`` keeps its whole stored row; a node at distance ``hops`` (the rim) keeps
one entry, (r, r).  The relabelling preserves order, so a kept row is summed in the order of the full graph; a kept
row's neighbours are all in the block; a rim row only feeds rows whose output nobody reads.  For a model of ``hops``
node-attention layers the rows ``seed_pos`` of every output on the block are therefore the rows ``seeds`` of the
full-graph outputs, with the model code unchanged::

    blk = ego_block(graphs, seeds, hops=1)
    logits, embed, att = model.forward([blk.take(x)] * P, blk.graphs)      # rows blk.seed_pos answer the seeds

:func:`predict` runs eval inference block by block, :class:`MiniBatchTrainer` the training step of ``HANTrainer`` on
the block of each batch.  Fan-out can be bounded beforehand (``metapath_graph(top_k=)``, ``metapath_sample(fanout=)``:
one deterministic cut of the graph) or per block: ``ego_block(..., fanout=f, seed=s)`` keeps in every row closer than
``hops`` its self entries and a random ``f`` of its other entries, drawn on the GPU, so a block holds at most
``B * prod(P * f)`` nodes whatever the degrees are, and every training step sees another subset.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import csr, layers, ops, rng
from .base_gattn import TFAdam
from .features import SparseFeatures, as_features
from .graph import CSRGraph, as_graph

CHUNK = 1024       # input rows with more entries are walked and copied in chunks of this many, a wave each


@dataclass
class EgoBlock:
    """nodes (n_b,) int64 ascending global ids; level (n_b,) int32 breadth-first distance from the seed set over the
    union of the graphs (seeds 0); seed_pos (B,) int64 with nodes[seed_pos[i]] == seeds[i]; graphs: P CSRGraphs
    n_b x n_b (module docstring); n: the nodes of the graphs the block was cut from."""
    nodes: torch.Tensor
    level: torch.Tensor
    seed_pos: torch.Tensor
    graphs: list
    n: int

    def take(self, x):
        """What the block's nodes hold of `x`: x[nodes] of a dense (N, ...) / (1, N, F) tensor -- features, labels,
        masks --, x.take(nodes) of sparse features (a SparseFeatures or a torch sparse tensor)."""
        x = as_features(x)
        if isinstance(x, SparseFeatures):
            if x.n_rows != self.n:
                raise ValueError(f"features have {x.n_rows} rows, the block was cut from {self.n} nodes")
            return x.take(self.nodes)
        if x.dim() == 3 and x.shape[0] == 1:
            x = x[0]
        if x.dim() < 1 or x.shape[0] != self.n:
            raise ValueError(f"expected a per-node tensor with {self.n} rows, got shape {tuple(x.shape)}")
        return x.index_select(0, self.nodes.to(x.device))


def _host_seeds(seeds, n):
    """Seeds given on the host as a checked int64 array: 1-D integers, B >= 1, distinct, inside [0, n)."""
    s = np.asarray(seeds)
    if s.size == 0:
        raise ValueError("seeds: empty")
    if s.ndim != 1 or s.dtype.kind not in "iu":
        raise ValueError(f"seeds: expected a 1-D integer array of node ids, got shape {s.shape} {s.dtype}")
    s = s.astype(np.int64)
    if int(s.min()) < 0 or int(s.max()) >= n:
        raise ValueError(f"seeds outside [0, {n}): [{int(s.min())}, {int(s.max())}]")
    if np.unique(s).size != s.size:
        raise ValueError("seeds: repeated node ids")
    return s


def _is_int(x) -> bool:
    return isinstance(x, (int, np.integer)) and not isinstance(x, (bool, np.bool_))


def _check_fanout(fanout, hops: int):
    """None, or the fan-out of every level 0 .. hops - 1 as a list of ints >= 1."""
    if fanout is None:
        return None
    fan = list(fanout) if isinstance(fanout, (list, tuple, np.ndarray)) else [fanout] * hops
    if len(fan) != hops:
        raise ValueError(f"fanout = {fanout!r}: expected one bound per level, {hops} for hops = {hops}")
    for f in fan:
        if not _is_int(f) or f < 1:
            raise ValueError(f"fanout = {fanout!r}: expected an integer >= 1 or a sequence of {hops} of them")
        if f > 2 ** 31 - 1:
            raise ValueError(f"fanout = {fanout!r}: beyond int32")
    return [int(f) for f in fan]


def _check_block_args(graphs, seeds, hops, fanout=None, seed=0):
    """Everything ego_block can refuse without a device: (graphs, n, host seeds or None for a device tensor, the
    fan-out per level or None)."""
    graphs = list(graphs)
    if isinstance(hops, bool) or int(hops) != hops or hops < 1:
        raise ValueError(f"hops = {hops!r}: expected an integer >= 1")
    fan = _check_fanout(fanout, int(hops))
    if not _is_int(seed):
        raise ValueError(f"seed = {seed!r}: expected an integer")
    if not graphs:
        raise ValueError("ego_block: no graphs")
    for p, g in enumerate(graphs):
        if not isinstance(g, CSRGraph):
            raise ValueError(f"graphs[{p}] is a {type(g)}, expected a CSRGraph")
        if g.n_rows != g.n_cols:
            raise ValueError(f"graphs[{p}] is {g.n_rows} x {g.n_cols}: an ego block needs square graphs")
        if g.n_rows != graphs[0].n_rows:
            raise ValueError(f"graphs[{p}] has {g.n_rows} nodes, graphs[0] has {graphs[0].n_rows}")
        if g.row_base != 0:
            raise ValueError(f"graphs[{p}] is a row shard (row_base = {g.row_base}): blocks are cut from whole graphs")
    n = graphs[0].n_rows
    if isinstance(seeds, torch.Tensor):
        if seeds.dim() != 1 or seeds.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"seeds: expected a 1-D int32 / int64 tensor, got {tuple(seeds.shape)} {seeds.dtype}")
        if seeds.numel() == 0:
            raise ValueError("seeds: empty")
        host = None
    else:
        host = _host_seeds(seeds, n)
    dev = graphs[0].device
    for p, g in enumerate(graphs):
        ops.require_gpu(g.rowptr, f"graphs[{p}]")
        if g.device != dev:
            raise ValueError(f"graphs[{p}] on {g.device}, graphs[0] on {dev}")
    if host is None:
        ops.require_gpu(seeds, "seeds")
        if seeds.device != dev:
            raise ValueError(f"seeds on {seeds.device}, the graphs on {dev}")
    return graphs, n, host, fan


def ego_block(graphs, seeds, hops: int = 1, fanout=None, seed: int = 0) -> EgoBlock:
    """The block of `seeds` (B >= 1 distinct node ids; an int32 / int64 tensor on the graphs' GPU, or a host array)
    in P square CSRGraphs over the same N nodes on one GPU (values optional, row_base 0), for a model of `hops` >= 1
    node-attention layers: see EgoBlock and the module docstring.  Raises ValueError, before any launch, for repeated,
    out-of-range or empty seeds, hops < 1, a non-square graph, graphs of different N, a row shard, and graphs or a
    seed tensor on the CPU (there is no CPU path).

    Launches: hops x P han_ego_expand (the graphs of a hop one after another on the stream), a scan of level >= 0
    for the local ids, then han_ego_count / han_ego_fill per graph (csrc/ego_block.hip).  HOST READS PER BLOCK: 2,
    whatever B, N, P and hops are -- n_b with the node list, then the P entry counts in one read -- and one more when
    the seeds come as a device tensor (their range and distinctness, in one read).  Rows longer than CHUNK entries
    are served by the input graph's own chunk table (CSRGraph.row_split), built on a graph's first block and cached
    with it.  Bitwise reproducible: integer stores only, every writer of a word writes the same value.

    `fanout` (None: the rule above, exactly) samples the rows: an int >= 1, or one per level 0 .. hops - 1 (seeds are
    level 0).  A row at level l < hops keeps its self entries (column == row; they do not count) and, of its d other
    entries, all when d <= fanout[l], else the fanout[l] of smallest (x, k): k the stored position in the row, x the
    first word of han_rand64(seed, stream 4 (p + 1), row, k) for graph number p (tests/rng_ref.py restates the hash;
    `seed` is taken mod 2^64).  Kept entries stay in stored order with their stored values, repeated entries are
    entries of their own, and levels are breadth-first over the sampled rows.  The block is therefore, bit for bit,
    ego_block(G', seeds, hops) of the graphs G' whose rows closer than hops are their selected entries -- the rows
    seed_pos of a model's outputs on it are the rows `seeds` of full-graph inference on G'.  Values are NOT reweighted
    (no importance weights): the attention softmax renormalises over the entries a row keeps.  Ties of x are decided
    exactly; the same (graphs, seeds, hops, fanout, seed) give the same block, bit for bit; the host reads stay as
    above.  Launches: hops x P han_ego_sample_expand, then han_ego_sample_count / han_ego_sample_fill per graph; a
    row beyond CHUNK entries is served by a 256-thread workgroup."""
    graphs, n, host, fan = _check_block_args(graphs, seeds, hops, fanout, seed)
    hops, P, dev = int(hops), len(graphs), graphs[0].device
    if host is not None:
        s = torch.as_tensor(host).to(dev)
    else:
        s = seeds.to(torch.int64)
        srt = torch.sort(s).values
        lo, hi, repeated = torch.stack([srt[0], srt[-1], (srt[1:] == srt[:-1]).any().to(torch.int64)]).tolist()
        if lo < 0 or hi >= n:
            raise ValueError(f"seeds outside [0, {n}): [{lo}, {hi}]")
        if repeated:
            raise ValueError("seeds: repeated node ids")
    splits = [g.row_split(CHUNK, CHUNK) for g in graphs]
    level = torch.full((n,), -1, dtype=torch.int32, device=dev)
    level[s] = 0
    dec = [ops.ego_sample_decision(g) for g in graphs] if fan is not None else None
    for h in range(hops):
        for p, (g, sp) in enumerate(zip(graphs, splits)):
            if fan is None:
                ops.ego_expand(g, level, h, sp)
            else:
                ops.ego_sample_expand(g, level, h, fan[h], seed, p, dec[p], sp)
    nodes = torch.nonzero(level >= 0).flatten()                               # host read 1: n_b
    n_b = nodes.numel()
    local = torch.full((n,), -1, dtype=torch.int32, device=dev)
    local[nodes] = torch.arange(n_b, dtype=torch.int32, device=dev)
    counts = torch.empty(P * n_b, dtype=torch.int64, device=dev)
    for p, g in enumerate(graphs):
        if fan is None:
            ops.ego_count(g.rowptr, nodes, counts[p * n_b:(p + 1) * n_b], level, hops)
        else:
            ops.ego_sample_count(nodes, counts[p * n_b:(p + 1) * n_b], level, hops, dec[p])
    ptr = csr.scan(counts)                                                    # the P row pointers end to end
    offs = ptr[::n_b].tolist()                                                # host read 2: the P entry counts
    out = []
    for p, (g, sp) in enumerate(zip(graphs, splits)):
        nnz = offs[p + 1] - offs[p]
        rowptr = ptr[p * n_b:(p + 1) * n_b + 1] - offs[p]
        colidx = torch.empty(nnz, dtype=torch.int32, device=dev)
        values = torch.empty(nnz, dtype=torch.float32, device=dev) if g.values is not None else None
        if nnz and fan is None:
            ops.ego_fill(g.rowptr, g.colidx, g.values, nodes, n, rowptr, colidx, values, level, hops, local, sp)
        elif nnz:
            ops.ego_sample_fill(g, nodes, rowptr, colidx, values, level, hops, local, seed, p, dec[p], sp)
        out.append(CSRGraph(rowptr, colidx, n_b, validate=False, values=values))
    return EgoBlock(nodes=nodes, level=level[nodes], seed_pos=local[s].long(), graphs=out, n=n)


# ---- using a block ---------------------------------------------------------------------------------------------------
def _model_hops(model) -> int:
    return 1 + len(model.extra)


def _inputs(model, xs, graphs):
    """(xs, graphs) as the model methods take them: features squeezed / converted once, graphs on the model's GPU."""
    if not model._built:
        raise RuntimeError("build the model first (model.build(...))")
    if model.partition is not None:
        raise NotImplementedError("ego blocks under a node partition are not supported")
    if model.semantic_mode == "metapath":
        raise ValueError('semantic="metapath": the weight of a meta-path is the mean of its scores over every node of the '
                         "graph; the mean over an ego block is another number, so blocks cannot answer for the full graph")
    dev = model.flat.device
    xs = [layers._squeeze_batch(x, f"xs[{i}]") for i, x in enumerate(xs)]
    xs = [x if isinstance(x, SparseFeatures) else x.contiguous() for x in xs]
    graphs = [as_graph(g, dev) for g in graphs]
    if len(xs) != len(graphs) or len(graphs) != model.P:
        raise ValueError(f"{len(xs)} feature inputs and {len(graphs)} graphs for a model of {model.P} meta-paths")
    for x, g in zip(xs, graphs):
        if x.shape[0] != g.n_rows:
            raise ValueError(f"graph has {g.n_rows} rows, features have {x.shape[0]}")
    return xs, graphs


def _take_each(blk: EgoBlock, xs):
    """blk.take of every input, an input shared by several meta-paths taken once."""
    done = {}
    return [done[id(x)] if id(x) in done else done.setdefault(id(x), blk.take(x)) for x in xs]


def predict(model, xs, graphs, rows=None, batch_size: int = 4096, fanout=None, seed: int = 0):
    """Eval inference of the nodes `rows` (default: all N; a 1-D integer tensor or array, repeats allowed), block by
    block: (logits (R, C), final_embed (R, D_out), att_val (R, P)) of exactly those rows, in their order -- the rows
    a full-graph model.inference returns for them.  hops is the model's node-attention layer count; the distinct
    rows are served in ascending batches of `batch_size` seeds, so peak memory follows the block, not N.  With
    `fanout` set (ego_block's fanout / seed) every block is sampled: APPROXIMATE inference -- the exact outputs of the
    graphs thinned to each block's selected entries, not those of the full graphs."""
    xs, graphs = _inputs(model, xs, graphs)
    _check_fanout(fanout, _model_hops(model))
    if isinstance(batch_size, bool) or int(batch_size) != batch_size or batch_size < 1:
        raise ValueError(f"batch_size = {batch_size!r}: expected an integer >= 1")
    dev, n, hops = model.flat.device, graphs[0].n_rows, _model_hops(model)
    if rows is None:
        uniq, inverse = torch.arange(n, device=dev), None
    else:
        r = rows if isinstance(rows, torch.Tensor) else torch.as_tensor(np.asarray(rows))
        if r.dim() != 1 or r.dtype.is_floating_point or r.dtype.is_complex or r.dtype == torch.bool:
            raise ValueError(f"rows: expected a 1-D integer array of node ids, got {tuple(r.shape)} {r.dtype}")
        uniq, inverse = torch.unique(r.to(device=dev, dtype=torch.int64), return_inverse=True)
    outs = ([], [], [])
    for b0 in range(0, uniq.numel(), int(batch_size)):
        blk = ego_block(graphs, uniq[b0:b0 + int(batch_size)], hops, fanout, seed)
        with torch.no_grad():
            M = model.node_level(_take_each(blk, xs), blk.graphs, 0.0, 0.0, False, ops.ACT_ELU)
            Z, att = model.semantic(M)
            logits = model.classify(Z)
        for o, t in zip(outs, (logits, Z, att)):
            o.append(t[blk.seed_pos])
    if not outs[0]:
        return (torch.empty((0, model.C), device=dev), torch.empty((0, model.D_out), device=dev),
                torch.empty((0, model.P), device=dev))
    res = tuple(torch.cat(o) for o in outs)
    return res if inverse is None else tuple(t[inverse] for t in res)


def epoch_batches(ids, batch_size: int, seed: int, epoch: int):
    """The batches of one epoch: `ids` (host array of node ids) in the order of a host permutation drawn from
    (seed, epoch), cut into runs of `batch_size`; the short last batch is kept.  Every id exactly once."""
    ids = np.asarray(ids, dtype=np.int64)
    if isinstance(batch_size, bool) or int(batch_size) != batch_size or batch_size < 1:
        raise ValueError(f"batch_size = {batch_size!r}: expected an integer >= 1")
    order = ids[np.random.default_rng([int(seed) & ((1 << 64) - 1), int(epoch)]).permutation(ids.size)]
    return [order[b0:b0 + int(batch_size)] for b0 in range(0, ids.size, int(batch_size))]


def block_seed(seed: int, step: int) -> int:
    """The ego_block seed of training step `step` of a trainer seeded `seed`: splitmix64(splitmix64(seed) + step),
    mod 2^64."""
    m = (1 << 64) - 1
    return rng._splitmix64((rng._splitmix64(int(seed) & m) + int(step)) & m)


class MiniBatchTrainer:
    """The training loop of HANTrainer on ego blocks: an epoch visits the training nodes once, in batches
    (epoch_batches), and every batch is one step of HANTrainer.train_step on the block of its seeds -- node_level
    (train=True), semantic, classifier_loss with the mask on seed_pos and weight 1 / B, backward, TFAdam.step -- with
    the trainer and the model code as they are.  Dropout draws are keyed by LOCAL node id: another, equally valid
    assignment than the full graph's (as under reorder's relabelling).  The dropout seed stream is the trainer's own
    (started from `seed`), so two trainers with equal seeds and equal initial parameters stay bit-equal.  Single
    process, eager (the shapes change per batch: nothing to capture).  `fanout` (ego_block's) samples every step's
    block afresh: the block seed of a step is block_seed(seed, steps done) -- splitmix64, apart from the dropout seed
    stream, which it does not consume: fanout=None, and a fan-out no degree exceeds, train bit for bit alike.
    evaluate() stays exact (unsampled blocks)."""

    def __init__(self, model, xs, graphs, labels, train_mask, val_mask=None, batch_size: int = 1024, lr=0.005,
                 l2_coef=0.001, attn_drop=0.6, ffd_drop=0.6, seed: int = 0, patience: int = 100, fanout=None,
                 objective="softmax"):
        """objective: HANTrainer's -- "sigmoid" takes (N, C) multi-hot labels, packed once (EgoBlock.take gathers the
        packed words like any dense row table), trains on the masked sigmoid cross-entropy and reports micro-F1 where
        "softmax" reports the accuracy."""
        from .trainer import check_objective, device_labels
        check_objective(objective, labels, model.Wc.shape[2])
        self.objective = objective
        self.model = model
        self.xs, self.graphs = _inputs(model, xs, graphs)
        model.direct_grads(True)
        dev = model.flat.device
        self.hops = _model_hops(model)
        self.fanout, self.steps_done = _check_fanout(fanout, self.hops), 0
        self.labels = device_labels(objective, labels, dev)
        self.train_mask = train_mask.to(device=dev, dtype=torch.uint8).contiguous()
        self.val_mask = (val_mask if val_mask is not None else train_mask).to(device=dev, dtype=torch.uint8).contiguous()
        self.train_ids = torch.nonzero(self.train_mask).flatten().cpu().numpy()
        if self.train_ids.size == 0:
            raise ValueError("train_mask selects no node")
        epoch_batches(self.train_ids[:1], batch_size, seed, 0)          # checks batch_size
        self.batch_size, self.seed = int(batch_size), int(seed)
        self.opt = TFAdam(model.flat, model.flat_grad, lr=lr, l2_coef=l2_coef)
        self._one = torch.ones((), dtype=torch.float32, device=dev)
        self.attn_drop, self.ffd_drop = float(attn_drop), float(ffd_drop)
        self._rng = {"seed": self.seed & ((1 << 64) - 1), "counter": 0}      # this trainer's rng._state
        self.epochs_done = 0
        self.patience = patience
        self.vlss_mn, self.vacc_mx, self.curr_step = float("inf"), 0.0, 0
        self.best_state = None
        self.last_counts = None

    def batches(self):
        """The seed batches of the next epoch (host arrays)."""
        return epoch_batches(self.train_ids, self.batch_size, self.seed, self.epochs_done)

    def train_step(self, seeds):
        """One optimiser step on the block of `seeds`; returns device scalars (loss, accuracy) over the seeds."""
        m = self.model
        blk = ego_block(self.graphs, seeds, self.hops, self.fanout, block_seed(self.seed, self.steps_done))
        self.steps_done += 1
        xs = _take_each(blk, self.xs)
        labels = blk.take(self.labels)
        mask = torch.zeros(blk.nodes.numel(), dtype=torch.uint8, device=labels.device)
        mask[blk.seed_pos] = 1
        saved = dict(rng._state)
        rng._state.update(self._rng)
        try:
            m.zero_grad_flat()
            with torch.enable_grad():
                M = m.node_level(xs, blk.graphs, self.attn_drop, self.ffd_drop, True, ops.ACT_ELU)
                Z, _ = m.semantic(M)
                res = m.classifier_loss(Z, labels, mask, 1.0 / blk.seed_pos.numel())
                loss, acc, _ = res
            self.last_counts = getattr(res, "counts", None)      # objective="sigmoid": [tp, fp, fn] of this batch
            loss.backward(self._one)
        finally:
            self._rng = dict(rng._state)
            rng._state.update(saved)
        self.opt.step()
        return loss.detach(), acc

    def evaluate(self, mask=None):
        """(loss, accuracy) over the nodes of `mask` (default: val_mask) with the current parameters, through
        predict: the masked softmax cross-entropy and accuracy of HANTrainer.eval_step, as device scalars."""
        mask = self.val_mask if mask is None else mask
        ids = torch.nonzero(mask.to(self.labels.device)).flatten()
        if ids.numel() == 0:
            raise ValueError("the mask selects no node")
        logits, embed, _ = predict(self.model, self.xs, self.graphs, ids, self.batch_size)
        if self.objective == "sigmoid":      # the masked sigmoid cross-entropy and micro-F1 of the rows, by the kernel
            with torch.no_grad():
                ones = torch.ones(ids.numel(), dtype=torch.uint8, device=embed.device)
                loss, f1, _ = layers.classifier_multilabel_any(embed.contiguous(), self.model.Wc, self.model.bc,
                                                               self.labels[ids].contiguous(), ones, 1.0 / ids.numel())
            return loss, f1
        labels = self.labels[ids].long()
        loss = torch.nn.functional.cross_entropy(logits, labels)
        return loss, (logits.argmax(1) == labels).to(torch.float32).mean()

    def epoch(self):
        """One pass over the training nodes, then the validation pair: (train loss, train accuracy -- the batch
        figures averaged over the training nodes --, val loss, val accuracy), device scalars.  With
        objective="sigmoid" the second and fourth are micro-F1, and the training one is formed ONCE from the counts
        tp / fp / fn summed over the batches: micro-F1 is a ratio of sums, not a mean of the batches' ratios (and one
        batch without a true positive must not turn the epoch's figure into NaN)."""
        tl = ta = 0.0
        counts = None
        for b in self.batches():
            loss, acc = self.train_step(b)
            tl, ta = tl + loss * (b.size / self.train_ids.size), ta + acc * (b.size / self.train_ids.size)
            if self.last_counts is not None:
                counts = self.last_counts.clone() if counts is None else counts + self.last_counts
        if counts is not None:
            ta = layers.micro_f1_of_counts(counts)
        self.epochs_done += 1
        vl, va = self.evaluate()
        return tl, ta, vl, va

    def early_stopping(self, val_loss: float, val_acc: float) -> bool:
        """HANTrainer.early_stopping (ex_acm3025.py:225-240): True to stop."""
        from .trainer import metric_improved
        acc_ok = metric_improved(val_acc, self.vacc_mx)      # a NaN micro-F1 is no improvement and is never stored
        if acc_ok or val_loss <= self.vlss_mn:
            if acc_ok and val_loss <= self.vlss_mn:
                self.best_state = self.model.flat.detach().clone()
            self.vacc_mx, self.vlss_mn = (val_acc if acc_ok else self.vacc_mx), min(val_loss, self.vlss_mn)
            self.curr_step = 0
            return False
        self.curr_step += 1
        return self.curr_step == self.patience

    def restore_best(self):
        if self.best_state is not None:
            self.model.flat.copy_(self.best_state)
