"""Layer library: the reference's ``utils/layers.py`` surface on the HIP kernels.

Same names, argument meaning and return values as the reference:

* :func:`attn_head`       -- utils/layers.py:7-46  (dense additive-mask form)
* :func:`attn_head_const_1` -- utils/layers.py:49-81 (HAN_nd ablation)
* :func:`sp_attn_head`    -- utils/layers.py:85-127 (SparseTensor form)
* :func:`SimpleAttLayer`  -- utils/layers.py:132-164

TensorFlow creates the variables inside each call; here they are passed in
``params`` (functional form) or owned by ``han_amd.gat.HeteGAT_multi`` (module
form).  The fast path used by the model is :class:`NodeLevelAttention`, which
runs all K heads of all P meta-paths through the K1/K2 kernels and writes the
heads straight into ``M[:, p, :]`` (models/gat.py:46,58-60).

There is no CPU implementation: every function raises on non-GPU tensors.
"""
from __future__ import annotations

import dataclasses
import functools
from typing import NamedTuple

import torch
import torch.nn.functional as F_torch

from . import ops, rng
from .dist import NodePartition
from .features import SparseFeatures, as_features, is_sparse_input
from .graph import as_graph

D = ops.D


def _act_code(activation):
    """Map the reference's `activation` argument to (kernel code, torch post-op)."""
    if activation is None:
        return ops.ACT_IDENTITY, None
    if activation in (F_torch.elu, torch.nn.functional.elu, "elu") or \
            isinstance(activation, torch.nn.ELU):
        return ops.ACT_ELU, None
    if activation == "identity":
        return ops.ACT_IDENTITY, None
    if callable(activation):
        return ops.ACT_IDENTITY, activation   # kernel emits the pre-activation; torch applies it
    raise ValueError(f"unsupported activation {activation!r}")


def _direct(p) -> bool:
    """True when parameter `p` asks the backward kernels to write straight into p.grad
    (set by HeteGAT_multi.direct_grads(True); see NodeLevelAttention.forward)."""
    return bool(getattr(p, "_han_direct_grad", False)) and p.grad is not None


def _same_tensor(ts) -> bool:
    """True when every entry is the same view of the same storage (the meta-paths share their features)."""
    t0 = ts[0]
    if any(isinstance(t, SparseFeatures) for t in ts):      # one sparse matrix for every meta-path, or no sharing
        return all(t is t0 for t in ts[1:])
    return all(t.data_ptr() == t0.data_ptr() and t.shape == t0.shape and t.stride() == t0.stride()
               and t.dtype == t0.dtype for t in ts[1:])


def _used_on(stream, *tensors):
    """Tensors allocated on one stream and read on another: tell the caching allocator, so that their memory is not
    handed out again before that stream is done with it."""
    for t in tensors:
        if t is not None:
            t.record_stream(stream)


def _unit_stride(x) -> bool:
    """Rows with contiguous elements (a SparseFeatures has no strides)."""
    return isinstance(x, SparseFeatures) or x.stride(-1) == 1


def _no_sparse_under_partition(partitioned: bool, *feature_lists):
    """Sparse features are single-process for now: under a node partition they fail loudly, before any launch,
    instead of falling into a dense path."""
    if partitioned and any(is_sparse_input(x) for xs in feature_lists if xs is not None for x in xs):
        raise NotImplementedError("sparse features under a node partition")


def _fork(streams):
    if streams is not None:
        cur = torch.cuda.current_stream()
        for st in streams:
            st.wait_stream(cur)


def _path_order(streams, graphs, how):
    """Order in which the per-meta-path chains are issued on their own streams (a captured epoch).  The chains are
    independent, so the results do not depend on it; what does is how the runtime lays the graph's branches on its
    queues (the first child of a fork continues on the parent's queue, the others start on queues of their own).
    "heavy" = largest graph first: measured with HANTrainer(overlap_eval="branch"), where the training forward's
    second chain otherwise starts ~50 us late (DBLP-like 0.88 -> 0.83 ms per epoch, ACM-like unchanged); the plain
    captured epoch keeps 0 .. P-1 (heavy-first there: ACM-like 0.394 -> 0.384 ms but DBLP-like 0.859 -> 0.902)."""
    P = len(graphs)
    if streams is None or how != "heavy":
        return list(range(P))
    return sorted(range(P), key=lambda p: (-int(graphs[p].nnz), p))


def _join(streams):
    if streams is not None:
        cur = torch.cuda.current_stream()
        for st in streams:
            cur.wait_stream(st)


def _each_path(streams, order, fn):
    """fn(p) for every meta-path, each on its own stream when there are path streams (LayerRun.streams, single GPU):
    the per-meta-path chains K1 -> K2 (forward) and rows -> cols -> score gradients -> dW (backward) are independent of
    each other, and at the size of the reference's data sets every kernel is a few microseconds on a few CUs -- side by
    side in a captured epoch they overlap instead of queueing (HANTrainer(use_graph=True)).  Scratch buffers are per
    path (ops.branch)."""
    for p in order:
        if streams is None:
            fn(p)
        else:
            with ops.branch(streams[p], f"@p{p}"):
                fn(p)


class _Ready:
    """A table that needs no exchange (same interface as the async exchange handles)."""

    def __init__(self, table):
        self.table = table

    def wait(self):
        return self.table


class LocalTable:
    """Table source of a meta-path whose gather table is the rows at hand (no node partition).  A table source has
    .graph (the CSR graph that indexes the table), .gid (global id of each table row, or None when row i is node i)
    and .exchange(table, tag) -> handle whose .wait() yields the gather table; the others are AllGatherTable,
    dist.HaloPlan and dist.MaskedBackwardPlan."""
    gid = None

    def __init__(self, graph):
        self.graph = graph

    def exchange(self, table, tag):
        return _Ready(table)


class AllGatherTable(LocalTable):
    """Table source of a meta-path without locality under a node partition: every rank's whole shard."""

    def __init__(self, part: NodePartition, graph):
        self.part, self.graph = part, graph

    def exchange(self, table, tag):
        return self.part.all_gather_rows_async(table, tag)


def stash_key(step, flat):
    """What must not have changed between the eval forward that stashed a training projection and the training forward
    that takes it: Adam's step count (the native Adam step writes `flat` without touching its version counter), the
    version counter of the flat parameter buffer (every torch-side write bumps it, through any view), and the
    buffer's address (nn.Module.to() and friends re-create it)."""
    return (int(step), int(flat._version), int(flat.data_ptr()))


class SharedProjection:
    """HANTrainer(shared_projection=...): inside epoch() the eval forward projects X with the parameters the NEXT
    training forward projects it with again, so its K1 runs as ops.project_fwd_both -- the eval tables plus, under the
    next step's seeds (rng.peek_seeds) and dropout rates, the training tables H / f1 / f2 / keep of every meta-path --
    and the training tables wait here.  The next training forward draws its seeds as always and takes them in place of
    its own ops.project_fwd_multi iff everything they depend on is what it would use itself (take()); they are
    byte for byte what that call computes.  A stash that is not taken is freed, and the ordinary call runs.
    The stash holds P x (N x 64 x 4 B + 2 x N x 8 x 4 B + N x F B): 4 x (256 + 64 + 256) MB at N = 1M, P = 4, F = 256."""

    def __init__(self, flat_of, step_of):
        self._flat_of, self._step_of = flat_of, step_of      # callables: the model's flat buffer, Adam's step count
        self.armed = None      # the training dropout rate while epoch() runs its eval forward, else None
        self._stash = None
        self.taken = 0         # training forwards that ran from a stash (tests, bench diagnostics)

    def key(self):
        return stash_key(self._step_of(), self._flat_of())

    @staticmethod
    def stash_bytes(N, F, P):
        return P * (N * D * 4 + 2 * N * 8 * 4 + N * F + 128)

    def drop(self):
        self._stash = None

    def eval_forward(self, X, W, a1, a2, b1, b2, row_offset, tdt):
        """The eval tables (H, f1, f2) of all meta-paths, the next step's training tables stashed -- or None where
        the combined kernel does not apply (nothing ran: the caller makes the ordinary eval call)."""
        self._stash = None
        P = W.shape[0]
        seeds = rng.peek_seeds(P)
        got = ops.project_fwd_both(X, W, a1, a2, b1, b2, self.armed, self.armed, seeds, row_offset=row_offset,
                                   table_dtype=tdt)
        if got is None:
            return None
        self._stash = (self.key(), X, float(self.armed), tuple(seeds), int(row_offset), tdt, got[0])
        return got[1]

    def take(self, X, in_drop, seeds, row_offset, tdt):
        """The stashed (H, f1, f2, keeps) for exactly this training projection, or None; the stash is gone either way."""
        st, self._stash = self._stash, None
        if st is None:
            return None
        key, Xs, drop, sds, off, tdt_s, tables = st
        if (Xs is X and drop == float(in_drop) and sds == tuple(int(v) for v in seeds) and off == int(row_offset)
                and tdt_s == tdt and key == self.key()):
            self.taken += 1
            return tables
        return None


@dataclasses.dataclass(frozen=True, eq=False)
class LayerRun:
    """How one call of NodeLevelAttention / WideHeadAttention is to run (built by gat.HeteGAT_multi.node_level)."""
    train: bool
    seeds: tuple                      # one dropout seed per meta-path
    act: int                          # kernel activation code (ops.ACT_*)
    in_drop: float = 0.0              # as asked for; what runs is drop_in / drop_coef (0 when not training)
    coef_drop: float = 0.0
    seed_dev: torch.Tensor | None = None       # device seed word of a captured step (han_hip.h "Seeds")
    part: NodePartition | None = None
    graphs_t: tuple | None = None     # the P transposed graphs of the backward (built on demand when None)
    layer: int = 0
    group: int = 0                    # head group (wide heads: head) of the layer; names the exchange tables
    table_dtype: torch.dtype = torch.float32   # storage of the H / g tables (float32 | bfloat16)
    plans_f: list | None = None       # per meta-path dist.HaloPlan or None (all-gather): forward / backward tables
    plans_b: list | None = None
    xs_full: tuple | None = None      # the features of ALL rows: replicated projection under a partition
    masked_bwd: list | None = None    # per meta-path dist.MaskedBackwardPlan, or None (the full pass)
    zero_rows: bool = False           # at most half of the loss rows are live and this is the only node-attention layer: the backward gather honours z (HAN_FLAG_K2_ZERO_ROWS)
    streams: list | None = None       # one stream per meta-path (_each_path)
    side_stream: torch.cuda.Stream | None = None   # dW beside the next meta-path's backward gather (NodeLevelAttention.backward)
    path_order: str | None = None     # _path_order
    overlap: object = None            # trainer._EvalBranch riding in this call's fork / join sections
    coef_sink: list | None = None     # receives per meta-path the coefficients of this call as data -- (E,K), or their
    coef_mean: bool = False           # head mean (E,) with coef_mean (return_coef of layers.py:43-44 / models/gat.py:143-172; single GPU only)
    fold_sink: list | None = None     # HeteGAT_multi.fold_k3: receives this call's FoldTail when its row-local backward may run in the K3 backward
    live_bwd: object = None           # LiveBackwardPlan (HANTrainer(live_backward=...)): the backward visits only the rows the loss reaches
    live_fwd: object = None           # LiveForwardPlan (HANTrainer(live_forward=...)): K2 computes only the rows the caller reads of M
    live_sink: list | None = None     # receives live_fwd when this call ran over it (a training call may decline: NodeLevelAttention.forward)
    fused_scores: object = "auto"     # HeteGAT_multi.fused_scores: the backward gather also takes the score-parameter gradients (ops.node_attn_bwd_cols_scores)
    shared_proj: object = None        # SharedProjection (HANTrainer(shared_projection=...)): the eval forward's K1 also projects for the next training forward

    @functools.cached_property
    def multi(self) -> bool:
        return self.part is not None and self.part.active

    @functools.cached_property
    def row_offset(self) -> int:
        return self.part.row_start if self.part is not None else 0

    @functools.cached_property
    def drop_in(self) -> float:
        return float(self.in_drop) if self.train else 0.0

    @functools.cached_property
    def drop_coef(self) -> float:
        return float(self.coef_drop) if self.train else 0.0

    def tag(self, kind, p, *s):
        """Name of the persistent exchange table of this (layer, head group, meta-path[, slice])."""
        return (kind, self.layer, self.group, p) + s

    def transposed(self, graphs):
        return self.graphs_t or tuple(g.transpose() for g in graphs)

    def _source(self, plans, p, graph):
        if not self.multi:
            return LocalTable(graph)
        if plans is not None and plans[p] is not None:       # halo rows only
            return plans[p]
        return AllGatherTable(self.part, graph)                # the whole shard

    def source_f(self, p, graph):
        """Table source of meta-path p's forward table H."""
        return self._source(self.plans_f, p, graph)

    def source_b(self, p, graph_t, masked=True):
        """(table source, kind of exchange tag) of meta-path p's backward table [g | stats]."""
        if masked and self.masked_bwd is not None and self.masked_bwd[p] is not None:
            return self.masked_bwd[p], "bm"      # opt-in: only the live rows are read / travel
        if masked and self.live_bwd is not None:
            return self.live_bwd.source(p, graph_t), "bl"      # the entries with a live destination, and no other
        return self._source(self.plans_b, p, graph_t), "b"


class LiveBackwardPlan:
    """Set-up-time plan of a backward that visits only the rows the loss reaches (HANTrainer(live_backward=...); single
    process, one node-attention layer): with a row-local classifier and K3, dZ_i, dM_i and g_i are exactly zero for every
    node i outside the train mask, which never changes.  `live`: the ascending int32 ids of the masked-in rows -- the row
    list of the K3 backward (ops.sem_attn_bwd_rows(live=...)); `graphs_t`: per meta-path the transposed graph with only
    the entries whose destination is live (CSRGraph.with_live_columns) -- the gather walks these and never meets a dead
    entry, so rows of the [g | stats] tables outside `live` are never read and need not be written; df1(K): per
    meta-path a persistent (N,K) buffer, zeroed once: the K3 backward writes its live rows, and the dead rows, which
    the gather's write_src and score_param_bwd read for every source row, stay the zeros they are in the full backward."""

    def __init__(self, graphs_t, train_mask):
        mask = train_mask != 0
        self.live = torch.nonzero(mask).flatten().to(torch.int32).contiguous()
        self.full_t = tuple(graphs_t)
        self.graphs_t = tuple(g.with_live_columns(mask) for g in graphs_t)
        self._sources = tuple(LocalTable(g) for g in self.graphs_t)
        self.n_rows = int(mask.numel())
        self._df1 = {}

    def source(self, p, graph_t):
        """Table source of meta-path p's live graph; `graph_t` is the transposed graph the step would gather over, which
        must be the one the plan was built from."""
        if graph_t is not self.full_t[p]:
            raise RuntimeError("live_backward: the model runs on other graphs than the trainer's; the live transposed "
                               "graphs were built from those (HANTrainer(live_backward=False) for free-form use)")
        return self._sources[p]

    def df1(self, K):
        if K not in self._df1:
            self._df1[K] = [torch.zeros((self.n_rows, K), dtype=torch.float32, device=self.live.device)
                            for _ in self.graphs_t]
        return self._df1[K]


class LiveForwardPlan:
    """Set-up-time plan of a forward that computes only the rows its caller reads (HANTrainer(live_forward=...); single
    process, one node-attention layer): the loss and the metrics of a step are sums over a mask that never changes,
    and K3 and the classifier are row-local, so row i of M, Z and the logits -- and of lse, aggp, tsum and beta, which
    only the live backward reads, at live rows -- matters only for i in the mask.  K1 still projects every row (H is
    the gather table).  `live`: the ascending int32 ids of the masked-in rows, the row list of the classifier
    (ops.classifier_loss(live=...)); subset(graph): per graph the bins and the split restricted to the rows
    (ops.RowSubset, computed on first use and kept); K3 runs over `live` too (ops.sem_attn_fwd(live=...)).  M, Z and the
    logits stay full-size and node-indexed; their
    other rows are uninitialised memory that nothing may sum over.  Whole-graph embeddings and logits remain what
    inference / predict return: those paths never take a plan.  backward: the LiveBackwardPlan over the same rows, or
    None -- a training forward runs over the list only in a step whose backward is that plan's row-list fold."""

    def __init__(self, graphs, mask, backward=None):
        self.mask = mask != 0
        self.backward = backward
        if backward is not None and not torch.equal(backward.live.to(self.mask.device), torch.nonzero(self.mask).flatten().to(torch.int32)):
            raise ValueError("LiveForwardPlan: `backward` lists other rows than `mask`")
        self.live = torch.nonzero(self.mask).flatten().to(torch.int32).contiguous()
        self.graphs = tuple(graphs)
        self.n_rows = int(self.mask.numel())
        self._subsets = [None] * len(self.graphs)

    def subset(self, graph):
        for p, g in enumerate(self.graphs):
            if g is graph:
                if self._subsets[p] is None:
                    self._subsets[p] = ops.RowSubset(g, self.mask, self.live)
                return self._subsets[p]
        raise RuntimeError("live_forward: the model runs on other graphs than the trainer's; the row lists were built "
                           "from those (HANTrainer(live_forward=False) for free-form use)")


class FoldTail:
    """Hand-over between NodeLevelAttention and SemanticAttention when M goes from the one straight into the other
    (HeteGAT_multi.fold_k3): the K3 backward then runs the row-local half of the K2 backward of every meta-path in its
    epilogue (ops.sem_attn_bwd_rows) -- dM is never written or read back -- and leaves the [g | stats] tables, df1 and dc
    here for NodeLevelAttention.backward, which goes on from the exchange of the tables.  Valid only while M has no
    other consumer: NodeLevelAttention.backward raises when the gradient it receives is not the placeholder the K3
    backward returned (_no_grad_of) -- autograd has then added another consumer's gradient to it."""
    __slots__ = ("saved", "c", "dc", "act", "K", "FP", "gs", "df1", "live")

    def __init__(self, saved, c, dc, act, K, FP, live=None):
        self.saved, self.c, self.dc, self.act, self.K, self.FP = saved, c, dc, act, K, FP
        self.live = live               # LiveBackwardPlan or None: the K3 backward runs over its row list
        self.gs = self.df1 = None      # filled by SemanticAttention.backward


_ZERO: dict = {}


def _no_grad_of(M):
    """The gradient a folded K3 backward returns for M: zeros that take no memory and no launch (one cached scalar per
    device, expanded); NodeLevelAttention.backward does not read it."""
    z = _ZERO.get(M.device)
    if z is None:
        z = _ZERO[M.device] = torch.zeros((), dtype=M.dtype, device=M.device)
    return z.expand(M.shape)


class _SavedPath(NamedTuple):
    """Backward state of one meta-path (NodeLevelAttention) or one column slice of it (WideHeadAttention: f1 / f2 are
    the head's totals).  The output rows the backward inverts the activation on are not here: M is kept through
    ctx.save_for_backward (version-checked by autograd, no reference cycle)."""
    H: torch.Tensor
    f1: torch.Tensor
    f2: torch.Tensor
    lse: torch.Tensor
    aggp: torch.Tensor
    tsum: torch.Tensor
    R: torch.Tensor | None
    keep: torch.Tensor | None = None


def _paths_in(Xin, xs, P):
    """(Xin, xs): layers >= 1 read meta-path p's input from the previous layer's output, Xin[:, p, :]."""
    if Xin is None:
        return None, xs
    Xin = Xin.contiguous()
    return Xin, tuple(Xin[:, p, :] for p in range(P))


def _residual_fwd(run, x, Wr, br, a1, a2, b1, b2, seed):
    """utils/layers.py:38-40: conv1d(seq, F', 1) of the DROPPED input -- the head's seed gives the same per-head
    input-dropout draws as for H; the projected rows are not dropped.  (The score vectors only ride along.)"""
    R, _, _ = ops.project_fwd(x, Wr, a1, a2, b1, b2, in_drop=run.drop_in, fts_drop=0.0, seed=seed,
                              row_offset=run.row_offset, seed_dev=run.seed_dev)
    return R + br


def _residual_g(gs, K, FP, dtype):
    """Residual: d(pre) = g, the fp32 rows of the fused backward table."""
    return ops.gs_views(gs, K, FP, dtype)[0].to(torch.float32).contiguous()


def _residual_bwd(run, x, g32, Wr, K, FP, seed, dWr, want_dx):
    """g flows into Wr (written to dWr) and, with want_dx, into the input (returned)."""
    ops.project_bwd(x, g32, K, FP, in_drop=run.drop_in, seed=seed, row_offset=run.row_offset,
                    seed_dev=run.seed_dev, out=dWr)
    if want_dx:
        return ops.project_bwd_input(g32, Wr.contiguous(), K, FP, in_drop=run.drop_in, seed=seed,
                                     row_offset=run.row_offset, seed_dev=run.seed_dev)


def _sink_coefs(run, graph, f1, f2, seed):
    if run.coef_sink is None:
        return
    if run.multi:
        raise NotImplementedError("return_coef is not provided under a node partition")
    run.coef_sink.append(ops.node_attn_coefs(graph, f1, f2, coef_drop=run.drop_coef, seed=seed,
                                             row_offset=run.row_offset, mean_heads=bool(run.coef_mean),
                                             seed_dev=run.seed_dev))


class NodeLevelAttention(torch.autograd.Function):
    """K1 + K2 for every meta-path: (X_p, graph_p) -> M (N, P, D).

    forward(Xin, W (P,F,D), a1 (P,K,F'), b1 (P,K), a2, b2, c (P,D), Wr, br, xs, graphs, run)
      Wr, br  None, or the residual connection of utils/layers.py:38-40 for layers whose
              input width differs from the head width: Wr (P,F,D) = the K heads'
              conv1d(seq, F', 1) kernels side by side, br (P,D) their biases; the term
              dropout_k(X) @ Wr_k + br_k is added before the activation
      Xin     None for the first layer; for layers >= 1 (models/gat.py:48-57) the
              previous layer's output (N,P,F): meta-path p reads Xin[:, p, :] and the
              backward returns dXin
      xs      tuple of P feature tensors (N,F) (no gradient: they are inputs);
              ignored when Xin is given
      graphs  tuple of P CSRGraph (rows = local destinations)
      run     LayerRun
    """

    @staticmethod
    def forward(ctx, Xin, W, a1, b1, a2, b2, c, Wr, br, xs, graphs, run):
        P = len(graphs)
        Xin, xs = _paths_in(Xin, xs, P)
        _no_sparse_under_partition(run.part is not None, xs, run.xs_full)
        K, FP = a1.shape[1], a1.shape[2]
        part, multi, train = run.part, run.multi, run.train
        in_drop, coef_drop, row_offset, seed_dev, tdt = run.drop_in, run.drop_coef, run.row_offset, run.seed_dev, run.table_dtype
        N = xs[0].shape[0]
        M = torch.empty((N, P, D), dtype=torch.float32, device=W.device)
        # THE place that decides whether this call's backward is the row-list fold (FoldTail with `live` set)
        fold = (run.fold_sink is not None and train and W.is_cuda and Wr is None and run.streams is None
                and tdt == torch.float32)
        fold_live = run.live_bwd if (fold and run.masked_bwd is None) else None
        # ... and whether K2 computes only the listed rows of M (LiveForwardPlan).  An eval call has no backward.  A
        # training call does so only when its backward is that fold over the SAME rows: every other backward reads M
        # and aggp of every row and sums dc over all of them, and one unwritten row would corrupt a gradient.
        live_f = run.live_fwd if (W.is_cuda and not multi and Wr is None and run.coef_sink is None) else None
        if live_f is not None and train and (fold_live is None or fold_live is not live_f.backward):
            live_f = None
        if live_f is not None and run.live_sink is not None:
            run.live_sink.append(live_f)
        saved = [None] * P
        srcs = [run.source_f(p, graphs[p]) for p in range(P)]
        # all projections first, each table's exchange started as soon as it exists:
        # the exchange of meta-path p+1.. overlaps the node attention of meta-path p
        proj = [None] * P
        xs_full = run.xs_full if (multi and Xin is None) else None
        # the reference feeds ONE feature matrix to every meta-path (ex_acm3025.py:86): all P projections then go
        # through ONE call -- the eval forward of long inputs as one fused launch that reads, splits and stages
        # every X tile once for four meta-paths (ops.project_fwd_multi)
        replicated = [xs_full is not None and isinstance(s, AllGatherTable) for s in srcs]
        pj = [None] * P
        shared = xs_full if all(replicated) else (xs if not any(replicated) else None)
        streams = run.streams if (not multi and run.streams is not None and len(run.streams) >= P) else None
        # the backward runs dW beside the next meta-path's gather (cols_path); the forward stays one chain
        side = run.side_stream if (streams is None and not multi and train and P > 1 and W.is_cuda) else None
        _fork(streams)
        # HANTrainer(overlap_eval=True): the eval forward's K1 + K2 as one more branch of this fork / join section
        overlap = run.overlap if (train and run.group == 0) else None
        if overlap is not None:
            overlap.node_level()
        if streams is None and P > 1 and shared is not None and _same_tensor(shared) and W.is_contiguous() and _unit_stride(shared[0]):
            full = all(replicated)
            off = 0 if full else row_offset
            # HANTrainer(shared_projection=...): the eval forward of an epoch also projects for the next training
            # forward, which then finds its tables waiting (SharedProjection; the same bytes either way)
            sp, got = run.shared_proj if seed_dev is None else None, None
            if sp is not None and train:
                got = sp.take(shared[0], in_drop, run.seeds, off, tdt)
            elif sp is not None and sp.armed is not None:
                ev = sp.eval_forward(shared[0], W, a1, a2, b1, b2, off, tdt)
                got = ev + ([None] * P,) if ev is not None else None
            Hs, f1s, f2s, keeps = got if got is not None else ops.project_fwd_multi(
                shared[0], W, a1, a2, b1, b2, in_drop=in_drop, fts_drop=in_drop, seeds=[int(v) for v in run.seeds],
                row_offset=off, table_dtype=tdt, seed_dev=seed_dev, want_keep=True)
            pj = [(Hs[p], f1s[p], f2s[p], keeps[p]) for p in range(P)]

        def project_path(p):
            seed = int(run.seeds[p])
            # replicated projection: every rank holds the features of ALL rows and projects the whole
            # table itself instead of receiving (G-1)/G of it -- a point-to-point xGMI link moves a
            # 256-B row slower than K1 recomputes it (dist.replication_policy).  Masks are keyed by
            # global row ids, so the rows are bit-identical to what their owners compute.
            X, off = (xs_full[p], 0) if replicated[p] else (xs[p], row_offset)
            # training: the forward also writes the keep table of its per-head input dropout, which dW
            # reads instead of regenerating the draws (None for shapes without a table)
            H, f1, f2, keep = pj[p] if pj[p] is not None else ops.project_fwd(
                X, W[p], a1[p], a2[p], b1[p], b2[p], in_drop=in_drop, fts_drop=in_drop, seed=seed,
                row_offset=off, table_dtype=tdt, seed_dev=seed_dev, want_keep=True)
            if replicated[p]:
                handle, r0, r1 = _Ready(H), part.row_start, part.row_end
                H, f1, f2 = H[r0:r1], f1[r0:r1], f2[r0:r1]
                if keep is not None:      # the local rows of the table (+ its slack) when they form a table themselves
                    Fw = X.shape[1]
                    kb_loc = ops.keep_bytes(r1 - r0, Fw, xs[p].stride(0), K, FP)
                    keep = keep[r0 * Fw:r0 * Fw + kb_loc] if kb_loc and (r0 * Fw) % 8 == 0 else None
            else:
                handle = srcs[p].exchange(H, run.tag("f", p))
            _sink_coefs(run, graphs[p], f1, f2, seed)
            # same seed -> the same per-head input-dropout draws as for H
            R = _residual_fwd(run, xs[p], Wr[p], br[p], a1[p], a2[p], b1[p], b2[p], seed) if Wr is not None else None
            proj[p] = (H, f1, f2, handle, R, keep)

        def attend_path(p):
            H, f1, f2, handle, R, keep = proj[p]
            _, sv = ops.node_attn_fwd(srcs[p].graph, handle.wait(), f1, a2[p], b2[p], c[p], out=M[:, p, :], train=train,
                                      coef_drop=coef_drop, fts_drop=in_drop, seed=int(run.seeds[p]), row_offset=row_offset,
                                      activation=run.act, table_gid=srcs[p].gid, res=R, seed_dev=seed_dev,
                                      f2=None if multi else f2, **({} if live_f is None else {"rows": live_f}))
            if train:      # sv[0] is the OUTPUT view M[:, p, :]: kept through ctx.save_for_backward(M) below, not here
                saved[p] = _SavedPath(H, f1, f2, *sv[1:], R, keep)

        order = _path_order(streams, graphs, run.path_order)
        _each_path(streams, order, project_path)
        _each_path(streams, order, attend_path)
        _join(streams)
        if overlap is not None:
            overlap.join()
        ctx.overlap = overlap
        del proj
        ctx.side = side
        ctx.run, ctx.xs, ctx.graphs = run, xs, graphs
        ctx.xin_shape = tuple(Xin.shape) if Xin is not None else None
        ctx.saved_per_p = saved
        # the per-meta-path tensors above were allocated on these streams: the backward must run each meta-path on
        # the SAME stream (the caching allocator ties a block to its allocation stream), whatever the model holds by then
        ctx.streams = streams
        ctx.has_res = Wr is not None
        # direct-gradient mode (HANTrainer): every parameter carries a pre-bound .grad slice of
        # the flat gradient buffer and is used once per step, so the backward kernels WRITE
        # their results there and autograd gets None (no copy / accumulate launches)
        plist = (W, a1, b1, a2, b2, c) + ((Wr, br) if Wr is not None else ())
        ctx.direct = tuple(p.grad for p in plist) if all(_direct(p) for p in plist) else None
        ctx.tail = None
        ctx.live_fwd = live_f is not None
        if fold:
            ctx.tail = FoldTail(saved, c, ctx.direct[5] if ctx.direct is not None else None, run.act, K, FP,
                                live=fold_live)
            run.fold_sink.append(ctx.tail)
        # M, the output, is backward state too (the pre-activation is recovered from it): saved through autograd, so
        # that an in-place change of M between forward and backward raises instead of giving wrong gradients
        ctx.save_for_backward(W, a1, b1, a2, b2, c, *((Wr,) if Wr is not None else ()), *((M,) if train else ()))
        return M

    @staticmethod
    def backward(ctx, dM):
        W, a1, b1, a2, b2, c = ctx.saved_tensors[:6]
        Wr = ctx.saved_tensors[6] if ctx.has_res else None
        run, xs, graphs = ctx.run, ctx.xs, ctx.graphs
        if not run.train:
            raise RuntimeError("NodeLevelAttention was run with train=False; no backward state")
        Mout = ctx.saved_tensors[-1]
        dWr = torch.empty_like(Wr) if Wr is not None else None
        dbr = torch.empty_like(c) if Wr is not None else None
        P = len(graphs)
        K, FP = a1.shape[1], a1.shape[2]
        tail, ctx.tail = ctx.tail, None
        folded = tail is not None and tail.gs is not None      # the K3 backward has run the row-local half (FoldTail)
        if ctx.live_fwd and not (folded and tail.live is not None):
            raise RuntimeError("live_forward: M holds only the listed rows, and the backward that reached it is not the "
                               "row-list fold (another consumer of M, or a K3 shape outside han_sem_attn_bwd_rows_live); "
                               "HANTrainer(live_forward=False) for such a model")
        if folded:
            if dM.data_ptr() != _no_grad_of(dM).data_ptr() or any(dM.stride()):
                raise RuntimeError("fold_k3: M has a consumer besides semantic(); its gradient cannot be folded into the K3 "
                                   "backward (set model.fold_k3 = False for free-form use of the model)")
        else:
            dM = dM.contiguous()
        graphs_t = run.transposed(graphs)
        in_drop, coef_drop, row_offset, seed_dev = run.drop_in, run.drop_coef, run.row_offset, run.seed_dev
        direct = ctx.direct
        if direct is not None:
            dW, da1, db1, da2, db2, dc = direct[:6]
            dWr, dbr = (direct[6], direct[7]) if Wr is not None else (None, None)
        else:
            dW = torch.empty_like(W)
            da1, da2 = torch.empty_like(a1), torch.empty_like(a2)
            db1, db2 = torch.empty_like(b1), torch.empty_like(b2)
            dc = tail.dc if folded else torch.empty_like(c)
        dXin = None
        if ctx.xin_shape is not None and ctx.needs_input_grad[0]:
            dXin = torch.empty(ctx.xin_shape, dtype=torch.float32, device=W.device)
        srcs = [run.source_b(p, graphs_t[p]) for p in range(P)]
        rows = [None] * P
        dres_in = []
        streams = ctx.streams       # the streams the forward ran (and allocated) on
        side = ctx.side
        _fork(streams)
        if ctx.overlap is not None:      # the eval forward's K3 + classifier beside the per-meta-path backward chains
            ctx.overlap.head()

        def rows_path(p):      # row-local halves first; their tables go out while we continue
            sv = ctx.saved_per_p[p]
            if folded:
                src, kind = srcs[p]
                rows[p] = (src.exchange(tail.gs[p], run.tag(kind, p)), tail.df1[p])
                return
            gs, df1, dcp = ops.node_attn_bwd_rows(dM[:, p, :], Mout[:, p, :], sv.aggp, sv.tsum, sv.f1, sv.lse, c[p],
                                                  activation=run.act, K=K, FP=FP,
                                                  table_dtype=sv.H.dtype, res=sv.R, dc_out=dc[p])
            if Wr is not None:
                g32 = _residual_g(gs, K, FP, sv.H.dtype)
                dbr[p] = dcp
                dx = _residual_bwd(run, xs[p], g32, Wr[p], K, FP, int(run.seeds[p]), dWr[p], dXin is not None)
                if dXin is not None:
                    dres_in.append(dx)
            src, kind = srcs[p]
            rows[p] = (src.exchange(gs, run.tag(kind, p)), df1)      # ONE fused [g | stats] table on the wire

        def cols_path(p):
            sv = ctx.saved_per_p[p]
            seed = int(run.seeds[p])
            gs_h, df1 = rows[p]
            src = srcs[p][0]
            cols_kw = dict(coef_drop=coef_drop, fts_drop=in_drop, seed=seed, src_offset=row_offset, dst_offset=0,
                           table_gid=src.gid, seed_dev=seed_dev,
                           **({"zero_rows": True} if run.zero_rows and srcs[p][1] != "bl" else {}))
            score_out = (da1[p], da2[p], db1[p], db2[p])
            if run.fused_scores is True or (run.fused_scores == "auto" and sv.H.is_cuda):
                # the gather also takes da1, da2, db1, db2 where the library has that form (ops.node_attn_bwd_cols_scores):
                # no second pass over H
                dH, df2, scored = ops.node_attn_bwd_cols(src.graph, gs_h.wait(), sv.H, sv.f2, df1, a1[p], a2[p],
                                                         scores_out=score_out, **cols_kw)
            else:
                dH, df2 = ops.node_attn_bwd_cols(src.graph, gs_h.wait(), sv.H, sv.f2, df1, a1[p], a2[p], **cols_kw)
                scored = False
            if not scored:
                ops.score_param_bwd(sv.H, df1, df2, K=K, FP=FP, out=score_out)
            rows[p] = None
            if side is not None and dXin is None:
                # dW(p) on the side stream (single GPU, eager training step on large graphs) beside the transposed-graph
                # gather of meta-path p + 1: the gather is bound by the memory fabric and leaves vector / matrix issue
                # slots that dW, bound by exactly those, can use -- 2.70 + 0.52 ms one after the other, 2.95 ms side by
                # side.  What was measured and is NOT done: the forward's K1 of meta-path p + 1 beside K2 of meta-path p
                # gains nothing (K2's blocks refill every slot they free, K1's 8-wave blocks with 40 KB of LDS wait:
                # 2.5 ms instead of 0.74, a higher stream priority changes nothing, and CU masks only move the same CU
                # time around: tools/cu_mask_probe.py); two K2 launches beside each other evict each other's gather
                # table from the Infinity Cache (four meta-path chains side by side: 40.7 ms per epoch against 35.5).
                side.wait_stream(torch.cuda.current_stream())
                with ops.branch(side, "@side"):
                    ops.project_bwd(xs[p], dH, K, FP, in_drop=in_drop, seed=seed,
                                    row_offset=row_offset, seed_dev=seed_dev, out=dW[p], keep=sv.keep)
                _used_on(side, dH)
                return
            ops.project_bwd(xs[p], dH, K, FP, in_drop=in_drop, seed=seed,
                            row_offset=row_offset, seed_dev=seed_dev, out=dW[p], keep=sv.keep)
            if dXin is not None:
                ops.project_bwd_input(dH, W[p], K, FP, out=dXin[:, p, :], in_drop=in_drop,
                                      seed=seed, row_offset=row_offset, seed_dev=seed_dev)
                if dres_in:
                    dXin[:, p, :] += dres_in[p]

        order = _path_order(streams, graphs, run.path_order)
        _each_path(streams, order, rows_path)
        _each_path(streams, order, cols_path)
        _join(streams)
        if ctx.overlap is not None:
            ctx.overlap.join()
            ctx.overlap = None
        if side is not None:
            torch.cuda.current_stream().wait_stream(side)
        ctx.saved_per_p = None
        if direct is not None:
            return (dXin,) + (None,) * 11
        return dXin, dW, da1, db1, da2, db2, dc, dWr, dbr, None, None, None


class WideHeadAttention(torch.autograd.Function):
    """K1 + K2 for ONE head wider than the 64 columns of a K1 / K2 row (hid_units > 64; models/gat.py:42-57 leaves
    the width free), every meta-path: the head runs as S = ceil(F'/64) column slices, each a K = 1, F' = 64 launch.

    What the slices of a head share is what makes them one head: the scores f1 / f2 (each slice's K1 epilogue gives
    its partial dot product, b1 / b2 ride in slice 0, the partials are added and K2 GATHERS f2 -- han_node_attn_fwd
    f2_src -- instead of recomputing it from its 64 columns), hence the coefficients, and the dropout draws keyed by
    the head: the per-head input dropout and the attention dropout (same seed, head index 0 in every slice).  The
    projected-row dropout is per column: slice s draws from its own stream (HAN_FLAG_FTS_SLICE).  The backward is the
    backward of the slices -- the softmax backward is linear in d alpha, so the slices' df1 / df2 add up -- with the
    totals in the places that need them (df1 into the transposed-graph pass, df2 into dH and the score gradients).

    forward(Xin, W (P,F,S*64), a1 (P,S*64), b1 (P,), a2 (P,S*64), b2 (P,), c (P,S*64), Wr, br, xs, graphs, run) -> M (N,P,S*64);
    columns beyond F' carry zero weights (their outputs are exactly act(0 + 0) and are cut off by the caller).
    run as for NodeLevelAttention.  Under a node partition every slice's table travels like a narrow head's (halo plan or
    all-gather, its own persistent exchange table) and so do the head's f2 totals (4 bytes per row); the forward is
    never replicated (xs_full is not used) and the backward exchanges one [g | stats] table per slice (always the full
    pass: masked_bwd is not used)."""

    @staticmethod
    def forward(ctx, Xin, W, a1, b1, a2, b2, c, Wr, br, xs, graphs, run):
        P = len(graphs)
        Xin, xs = _paths_in(Xin, xs, P)
        _no_sparse_under_partition(run.part is not None, xs, run.xs_full)
        S = W.shape[2] // D
        train = run.train
        in_drop, coef_drop, row_offset, seed_dev = run.drop_in, run.drop_coef, run.row_offset, run.seed_dev
        N, dev = xs[0].shape[0], W.device
        M = torch.empty((N, P, S * D), dtype=torch.float32, device=dev)
        zero1 = torch.zeros(1, dtype=torch.float32, device=dev)
        saved = []
        for p in range(P):
            seed = int(run.seeds[p])
            Ws = W[p].view(-1, S, D).permute(1, 0, 2).contiguous()          # (S,F,64)
            a1s, a2s, cs = a1[p].view(S, 1, D), a2[p].view(S, 1, D), c[p].view(S, D)
            src = run.source_f(p, graphs[p])
            Hs, Htabs, f1, f2, Rs = [], [], None, None, []
            for s_ in range(S):
                fl = ops.flag_fts_slice(s_)
                H, f1s, f2s = ops.project_fwd(xs[p], Ws[s_], a1s[s_], a2s[s_], b1[p:p + 1] if s_ == 0 else zero1,
                                              b2[p:p + 1] if s_ == 0 else zero1, in_drop=in_drop, fts_drop=in_drop,
                                              seed=seed, row_offset=row_offset, table_dtype=run.table_dtype,
                                              seed_dev=seed_dev, flags=fl)
                Hs.append(H)
                Htabs.append(src.exchange(H, run.tag("wf", p, s_)))
                f1 = f1s if f1 is None else f1 + f1s
                f2 = f2s if f2 is None else f2 + f2s
                Rs.append(_residual_fwd(run, xs[p], Wr[p].view(-1, S, D)[:, s_, :].contiguous(), br[p].view(S, D)[s_],
                                        a1s[s_], a2s[s_], zero1, zero1, seed) if Wr is not None else None)
            _sink_coefs(run, graphs[p], f1, f2, seed)
            f2_tab = src.exchange(f2, run.tag("wf2", p)).wait()      # the head's scores of every table row
            per_s = []
            for s_ in range(S):
                _, sv = ops.node_attn_fwd(src.graph, Htabs[s_].wait(), f1, a2s[s_], b2[p:p + 1], cs[s_],
                                          out=M[:, p, s_ * D:(s_ + 1) * D], train=train, coef_drop=coef_drop,
                                          fts_drop=in_drop, seed=seed, row_offset=row_offset, activation=run.act,
                                          table_gid=src.gid, res=Rs[s_], seed_dev=seed_dev, f2_src=f2_tab)
                if train:      # the output slice: ctx.save_for_backward(M)
                    per_s.append(_SavedPath(Hs[s_], f1, f2, *sv[1:], Rs[s_]))
            if train:
                saved.append(per_s)
        ctx.run, ctx.xs, ctx.graphs, ctx.S = run, xs, graphs, S
        ctx.xin_shape = tuple(Xin.shape) if Xin is not None else None
        ctx.saved_per_p = saved
        ctx.has_res = Wr is not None
        ctx.save_for_backward(W, a1, a2, c, *((Wr,) if Wr is not None else ()), *((M,) if train else ()))
        return M

    @staticmethod
    def backward(ctx, dM):
        W, a1, a2, c = ctx.saved_tensors[:4]
        Wr = ctx.saved_tensors[4] if ctx.has_res else None
        run, xs, graphs, S = ctx.run, ctx.xs, ctx.graphs, ctx.S
        if not run.train:
            raise RuntimeError("WideHeadAttention was run with train=False; no backward state")
        Mout = ctx.saved_tensors[-1]
        P, dev = len(graphs), W.device
        Fw = W.shape[1]
        dM = dM.contiguous()
        graphs_t = run.transposed(graphs)
        in_drop, coef_drop, row_offset, seed_dev = run.drop_in, run.drop_coef, run.row_offset, run.seed_dev
        dW = torch.empty((P, S, Fw, D), dtype=torch.float32, device=dev)
        da1, da2, dc = torch.empty_like(a1), torch.empty_like(a2), torch.empty_like(c)
        db1 = torch.empty((P,), dtype=torch.float32, device=dev)
        db2 = torch.empty((P,), dtype=torch.float32, device=dev)
        dWr = torch.empty((P, S, Fw, D), dtype=torch.float32, device=dev) if Wr is not None else None
        dXin = None
        if ctx.xin_shape is not None and ctx.needs_input_grad[0]:
            dXin = torch.zeros(ctx.xin_shape, dtype=torch.float32, device=dev)
        for p in range(P):
            per_s = ctx.saved_per_p[p]
            f1, f2 = per_s[0].f1, per_s[0].f2
            seed = int(run.seeds[p])
            a1s, a2s, cs = a1[p].view(S, 1, D), a2[p].view(S, 1, D), c[p].view(S, D)
            src = run.source_b(p, graphs_t[p], masked=False)[0]
            rows, df1 = [], None
            for s_ in range(S):       # row-local halves: g, the slice's share of df1
                sv = per_s[s_]
                gs, df1s, _ = ops.node_attn_bwd_rows(dM[:, p, s_ * D:(s_ + 1) * D], Mout[:, p, s_ * D:(s_ + 1) * D], sv.aggp,
                                                     sv.tsum, f1, sv.lse, cs[s_],
                                                     activation=run.act, K=1, FP=D, table_dtype=sv.H.dtype, res=sv.R,
                                                     dc_out=dc[p, s_ * D:(s_ + 1) * D])
                rows.append(src.exchange(gs, run.tag("wb", p, s_)))      # one [g | stats] table per slice
                df1 = df1s if df1 is None else df1 + df1s
                if Wr is not None:
                    dx = _residual_bwd(run, xs[p], _residual_g(gs, 1, D, sv.H.dtype), Wr[p].view(-1, S, D)[:, s_, :], 1, D,
                                       seed, dWr[p, s_], dXin is not None)
                    if dXin is not None:
                        dXin[:, p, :] += dx
            cols, df2 = [], None
            for s_ in range(S):       # transposed-graph halves with the head's df1; each returns its share of df2
                dH, df2s = ops.node_attn_bwd_cols(src.graph, rows[s_].wait(), per_s[s_].H, f2, df1, a1s[s_], a2s[s_],
                                                  coef_drop=coef_drop, fts_drop=in_drop, seed=seed, src_offset=row_offset,
                                                  dst_offset=0, table_gid=src.gid, seed_dev=seed_dev)
                cols.append((dH, df2s))
                df2 = df2s if df2 is None else df2 + df2s
            for s_ in range(S):
                H = per_s[s_].H
                dH, df2s = cols[s_]
                if S > 1:             # the kernel added its own df2 share times a2; the head's total belongs there
                    dH.addcmul_(df2 - df2s, a2s[s_])
                o1 = torch.empty((1,), dtype=torch.float32, device=dev) if s_ else db1[p:p + 1]
                o2 = torch.empty((1,), dtype=torch.float32, device=dev) if s_ else db2[p:p + 1]
                ops.score_param_bwd(H, df1, df2, K=1, FP=D, out=(da1[p].view(S, 1, D)[s_], da2[p].view(S, 1, D)[s_], o1, o2))
                ops.project_bwd(xs[p], dH, 1, D, in_drop=in_drop, seed=seed, row_offset=row_offset, seed_dev=seed_dev,
                                out=dW[p, s_])
                if dXin is not None:
                    Ws = W[p].view(-1, S, D)[:, s_, :].contiguous()
                    dXin[:, p, :] += ops.project_bwd_input(dH, Ws, 1, D, in_drop=in_drop, seed=seed,
                                                           row_offset=row_offset, seed_dev=seed_dev)
        ctx.saved_per_p = None
        fold = lambda t: t.permute(0, 2, 1, 3).reshape(P, Fw, S * D)
        return (dXin, fold(dW), da1, db1, da2, db2, dc, fold(dWr) if dWr is not None else None,
                dc.clone() if Wr is not None else None, None, None, None)


class SemanticAttention(torch.autograd.Function):
    """K3: M (N,P,D) -> (Z (N,D), beta (N,P)); utils/layers.py:152-159."""

    @staticmethod
    def forward(ctx, M, w_omega, b_omega, u_omega, *tail):
        """tail: nothing, or the FoldTail of the NodeLevelAttention call whose output M is (semantic_attention), and / or
        the LiveForwardPlan of a forward that computed only the plan's rows of M: K3 then runs over the same list."""
        M = M.contiguous()
        live = next((t for t in tail if isinstance(t, LiveForwardPlan)), None)
        Z, beta = ops.sem_attn_fwd(M, w_omega, b_omega, u_omega, **({} if live is None else {"live": live.live}))
        ctx.n_tail = len(tail)
        ctx.tail = next((t for t in tail if isinstance(t, FoldTail)), None)
        ctx.set_materialize_grads(False)      # no zero-filled gradient for beta (a fill launch per step)
        plist = (w_omega, b_omega, u_omega)
        ctx.direct = tuple(p.grad for p in plist) if all(_direct(p) for p in plist) else None
        ctx.save_for_backward(M, w_omega, b_omega, u_omega, beta)
        ctx.mark_non_differentiable(beta)
        return Z, beta

    @staticmethod
    def backward(ctx, dZ, _dbeta):
        M, w, b, u, beta = ctx.saved_tensors
        if dZ is None:
            dZ = torch.zeros((M.shape[0], M.shape[2]), dtype=M.dtype, device=M.device)
        tail, ctx.tail = ctx.tail, None
        none = (None,) * ctx.n_tail
        if tail is not None:      # the row-local K2 backward in this kernel's epilogue; None: not a shape of the fused kernel
            dc = tail.dc if tail.dc is not None else torch.empty_like(tail.c)
            r = ops.sem_attn_bwd_rows(M, w, b, u, beta, dZ.contiguous(),
                                      [(sv.aggp, sv.tsum, sv.f1, sv.lse) for sv in tail.saved], tail.c.contiguous(), dc,
                                      activation=tail.act, K=tail.K, FP=tail.FP, table_dtype=tail.saved[0].H.dtype,
                                      out=ctx.direct, **({} if tail.live is None else
                                                         {"live": tail.live.live, "df1_out": tail.live.df1(tail.K)}))
            if r is not None:
                tail.gs, tail.df1, tail.dc = r[0], r[1], dc
                if ctx.direct is not None:
                    return (_no_grad_of(M), None, None, None) + none
                return (_no_grad_of(M),) + tuple(r[2:]) + none
        dM, dw, db, du = ops.sem_attn_bwd(M, w, b, u, beta, dZ.contiguous(), out=ctx.direct)
        if ctx.direct is not None:
            return (dM, None, None, None) + none
        return (dM, dw, db, du) + none


class SemanticAttentionMean(torch.autograd.Function):
    """K3 as published (han.pdf eq. 7-9): M (N,P,D) -> (Z (N,D), beta (P,)), one weight per meta-path from the node
    means of the scores.  Every row of dM depends on every row of dZ, so nothing row-local (FoldTail, row lists)
    applies here."""

    @staticmethod
    def forward(ctx, M, w_omega, b_omega, u_omega):
        M = M.contiguous()
        Z, beta = ops.sem_attn_mean_fwd(M, w_omega, b_omega, u_omega)
        ctx.set_materialize_grads(False)
        plist = (w_omega, b_omega, u_omega)
        ctx.direct = tuple(p.grad for p in plist) if all(_direct(p) for p in plist) else None
        ctx.save_for_backward(M, w_omega, b_omega, u_omega, beta)
        ctx.mark_non_differentiable(beta)
        return Z, beta

    @staticmethod
    def backward(ctx, dZ, _dbeta):
        M, w, b, u, beta = ctx.saved_tensors
        if dZ is None:
            dZ = torch.zeros((M.shape[0], M.shape[2]), dtype=M.dtype, device=M.device)
        dM, dw, db, du = ops.sem_attn_mean_bwd(M, w, b, u, beta, dZ.contiguous(), out=ctx.direct)
        if ctx.direct is not None:
            return dM, None, None, None
        return dM, dw, db, du


class ClassifierLoss(torch.autograd.Function):
    """Fused classifier + masked softmax-CE (+ accuracy).
    models/gat.py:65-72, models/base_gattn.py:41-48,61-69.
    Returns (loss, accuracy, logits (N,C)); only `loss` is differentiable."""

    @staticmethod
    def forward(ctx, Z, Wc, bc, labels, mask, row_weight, *grad_mode):
        """grad_mode: nothing, or (grad enabled,), or (grad enabled, live): the int32 row list of a forward that
        computed only those rows of Z (LiveForwardPlan.live; None: every row)."""
        # an eval forward under torch.no_grad() must neither pay for the gradient half of the kernel nor, in
        # direct-gradient mode, WRITE Wc.grad / bc.grad.  needs_input_grad reports requires_grad whatever the grad
        # mode and the grad mode is off inside every forward(), so the caller passes the one it was called under
        # (classifier_loss_any); without it the inputs decide, as before
        need = any(ctx.needs_input_grad[:3]) and (not grad_mode or bool(grad_mode[0]))
        ctx.n_opt = len(grad_mode)
        ctx.set_materialize_grads(False)      # no zero-filled gradients for the accuracy / logits outputs
        # direct-gradient mode additionally assumes the loss is the root of backward()
        # (d loss = 1), which is how HANTrainer calls it
        ctx.direct = need and _direct(Wc) and _direct(bc)
        logits, loss_acc, grads = ops.classifier_loss(Z.contiguous(), Wc, bc, labels, mask,
                                                      row_weight, backward=need,
                                                      grad_out=(Wc.grad, bc.grad) if ctx.direct else None,
                                                      **({"live": grad_mode[1]} if len(grad_mode) > 1 else {}))
        ctx.grads = grads
        if ctx.direct or not need:      # views of the kernel's output pair: no clone launches (eval forward: nothing to differentiate)
            loss, acc = loss_acc[0:1].view(()), loss_acc[1:2].view(())
        else:
            loss, acc = loss_acc[0].clone(), loss_acc[1].clone()
        ctx.mark_non_differentiable(acc, logits)
        return loss, acc, logits

    @staticmethod
    def backward(ctx, dloss, _dacc, _dlogits):
        dZ, dWc, dbc = ctx.grads
        ctx.grads = None
        tail = (None,) * (3 + ctx.n_opt)
        if ctx.direct:
            return (dZ, None, None) + tail
        if dloss is None:
            return (None, None, None) + tail
        return (dZ * dloss, dWc * dloss, dbc * dloss) + tail


class MultiLabelResult(tuple):
    """What classifier_multilabel_any returns: the 3-tuple (loss, micro_f1, logits) -- the shape of
    classifier_loss_any's result, in length, indexing and unpacking -- with one attribute more: `counts`, the int64
    device tensor [tp, fp, fn] the metric was formed from (sums over ranks or batches, which micro-F1 itself is not:
    micro_f1_of_counts forms it from summed counts)."""

    def __new__(cls, loss, micro_f1, logits, counts):
        r = super().__new__(cls, (loss, micro_f1, logits))
        r.counts = counts
        return r

    loss = property(lambda self: self[0])
    micro_f1 = property(lambda self: self[1])
    logits = property(lambda self: self[2])


def micro_f1_of_counts(counts):
    """2 tp / (2 tp + fp + fn) in double, rounded to fp32, of an int64 tensor [tp, fp, fn] (models/base_gattn.py:90-92,
    algebraically); NaN for tp == 0, the reference's 0 / 0.  A few scalar torch ops on the device of `counts`."""
    c = counts.to(torch.float64)
    f1 = 2.0 * c[0] / (2.0 * c[0] + c[1] + c[2])
    return torch.where(counts[0] == 0, torch.full_like(f1, float("nan")), f1).to(torch.float32)


class MultiLabelClassifierLoss(torch.autograd.Function):
    """Fused classifier + masked sigmoid cross-entropy (+ micro-F1 and its counts).
    models/gat.py:65-72, models/base_gattn.py:50-59,71-94.
    Returns (loss, micro_f1, logits (N,C), counts (3,) int64); only `loss` is differentiable."""

    @staticmethod
    def forward(ctx, Z, Wc, bc, label_bits, mask, row_weight, *grad_mode):
        """grad_mode: as ClassifierLoss.forward -- nothing, (grad enabled,) or (grad enabled, live)."""
        need = any(ctx.needs_input_grad[:3]) and (not grad_mode or bool(grad_mode[0]))
        ctx.n_opt = len(grad_mode)
        ctx.set_materialize_grads(False)
        ctx.direct = need and _direct(Wc) and _direct(bc)
        logits, loss_acc, counts, grads = ops.classifier_multilabel(
            Z.contiguous(), Wc, bc, label_bits, mask, row_weight, backward=need,
            grad_out=(Wc.grad, bc.grad) if ctx.direct else None,
            **({"live": grad_mode[1]} if len(grad_mode) > 1 else {}))
        ctx.grads = grads
        if ctx.direct or not need:
            loss, f1 = loss_acc[0:1].view(()), loss_acc[1:2].view(())
        else:
            loss, f1 = loss_acc[0].clone(), loss_acc[1].clone()
        ctx.mark_non_differentiable(f1, logits, counts)
        return loss, f1, logits, counts

    @staticmethod
    def backward(ctx, dloss, _df1, _dlogits, _dcounts):
        dZ, dWc, dbc = ctx.grads
        ctx.grads = None
        tail = (None,) * (3 + ctx.n_opt)
        if ctx.direct:
            return (dZ, None, None) + tail
        if dloss is None:
            return (None, None, None) + tail
        return (dZ * dloss, dWc * dloss, dbc * dloss) + tail


class _ClassifierForward(torch.autograd.Function):
    """logits = (1/HC) sum_h (Z Wc[h] + bc[h]) (models/gat.py:65-72) by the HIP kernels, forward and backward
    (han_classifier_loss with an empty mask; han_classifier_bwd for a caller-supplied dlogits)."""

    @staticmethod
    def forward(ctx, Z, Wc, bc):
        N = Z.shape[0]
        labels = torch.zeros(N, dtype=torch.int32, device=Z.device)
        mask = torch.zeros(N, dtype=torch.uint8, device=Z.device)
        Z = Z.contiguous()
        logits, _, _ = ops.classifier_loss(Z, Wc, bc, labels, mask, 0.0, backward=False)
        ctx.save_for_backward(Z, Wc, bc)
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        Z, Wc, bc = ctx.saved_tensors
        return ops.classifier_bwd(Z, Wc, bc, dlogits.contiguous())


def classifier(Z, Wc, bc):
    return _ClassifierForward.apply(Z, Wc, bc)


K3_WIDTHS = (64, 128)      # embedding widths the TUNED K3 / classifier kernels are built for
K3_MAX_ATT = 256           # attention sizes of the tuned K3 kernels: multiples of 64 up to 256
MAX_CLASSES = 64           # classes of the fused single-launch classifier kernels (more: the three-kernel path)


def _pad_to(n: int) -> int:
    return 64 * ((n + 63) // 64)


SEMANTIC_MODES = ("node", "metapath")


def check_semantic(mode):
    if mode not in SEMANTIC_MODES:
        raise ValueError(f"semantic: expected one of {SEMANTIC_MODES}, got {mode!r}")
    return mode


def _semantic_attention_mean(M, w_omega, b_omega, u_omega):
    """mode="metapath" of semantic_attention: han.pdf eq. 7-9 on the kernels of sem_attn_mean.hip.  The zero-padding is
    exact here too (a padded column adds tanh(.) * 0 to every score, hence 0 to every mean)."""
    d, a = M.shape[2], w_omega.shape[1]
    dm, am = _pad_to(d), _pad_to(a)
    if dm not in ops.SEM_MEAN_D or am not in ops.SEM_MEAN_A or not 1 <= M.shape[1] <= ops.SEM_MEAN_MAX_P:
        raise NotImplementedError(
            f'semantic="metapath": D = {d}, A = {a}, P = {M.shape[1]} is outside the kernels\' shapes: D (padded to a '
            f"multiple of 64) in {ops.SEM_MEAN_D}, A (padded) in {ops.SEM_MEAN_A}, 1 <= P <= {ops.SEM_MEAN_MAX_P}")
    if dm == d and am == a:
        Z, beta = SemanticAttentionMean.apply(M.contiguous(), w_omega, b_omega, u_omega)
    else:
        Z, beta = SemanticAttentionMean.apply(
            torch.nn.functional.pad(M, (0, dm - d)), torch.nn.functional.pad(w_omega, (0, am - a, 0, dm - d)),
            torch.nn.functional.pad(b_omega, (0, am - a)), torch.nn.functional.pad(u_omega, (0, am - a)))
        Z = Z[:, :d]
    return Z, beta.expand(M.shape[0], -1)      # (N,P), stride 0 over the P device floats: every node's row is beta


def semantic_attention(M, w_omega, b_omega, u_omega, tail=None, live=None, mode="node"):
    """utils/layers.py:152-159 for any embedding width D and attention size A, always on the K3 kernels.
    Widths that are not multiples of 64 are zero-padded -- padded columns of w_omega / u_omega contribute
    tanh(.) * 0 = 0 to the scores and padded embedding columns are 0 -- which is exact.  D in {64, 128} with
    A <= 256 run the tuned kernels; anything wider (a last layer of 8 heads x 32, hid_units = [128],
    mp_att_size = 512, ...) the run-time-width kernels of sem_attn.hip (round 3: no torch branch is left).
    mode="metapath": the published form, one weight per meta-path (han.pdf eq. 7-9) -- the softmax is taken once, over the
    node means of the scores; the returned attention is that (P,) vector expanded to (N,P).  It needs every row of M,
    so it takes neither a FoldTail nor a row list."""
    if check_semantic(mode) == "metapath":
        if tail is not None or live is not None:
            raise ValueError('semantic="metapath" is not row-local: the mean runs over every node, and every row of dM '
                             "depends on every row of dZ; it takes no FoldTail and no row list")
        return _semantic_attention_mean(M, w_omega, b_omega, u_omega)
    d, a = M.shape[2], w_omega.shape[1]
    dm, am = _pad_to(d), _pad_to(a)
    if dm == d and am == a:      # tail: M is the output of the NodeLevelAttention call that made it (FoldTail); padded, it is not
        return SemanticAttention.apply(M.contiguous(), w_omega, b_omega, u_omega,
                                       *(t for t in (tail, live) if t is not None))
    Z, att = SemanticAttention.apply(
        torch.nn.functional.pad(M, (0, dm - d)), torch.nn.functional.pad(w_omega, (0, am - a, 0, dm - d)),
        torch.nn.functional.pad(b_omega, (0, am - a)), torch.nn.functional.pad(u_omega, (0, am - a)))
    return Z[:, :d], att


def classifier_any(Z, Wc, bc):
    """models/gat.py:65-72 for any embedding width and class count: always the HIP kernels (widths that are not
    multiples of 64 are zero-padded, which is exact)."""
    d = Z.shape[1]
    dm = _pad_to(d)
    if dm != d:
        Z, Wc = torch.nn.functional.pad(Z, (0, dm - d)), torch.nn.functional.pad(Wc, (0, 0, 0, dm - d))
    return classifier(Z, Wc, bc)


def classifier_loss_any(Z, Wc, bc, labels, mask, weight, live=None):
    """Classifier + masked softmax cross-entropy + accuracy (models/base_gattn.py:41-48,61-69) for any
    embedding width / class count; returns (loss, accuracy, logits).  live: the row list of a Z of which only those rows
    were computed (ops.classifier_loss(live=...): widths of 64 / 128 columns, at most 64 classes)."""
    d = Z.shape[1]
    dm = _pad_to(d)
    if live is not None:
        return ClassifierLoss.apply(Z, Wc, bc, labels, mask, weight, torch.is_grad_enabled(), live)
    if dm != d:
        Z, Wc = torch.nn.functional.pad(Z, (0, dm - d)), torch.nn.functional.pad(Wc, (0, 0, 0, dm - d))
    return ClassifierLoss.apply(Z, Wc, bc, labels, mask, weight, torch.is_grad_enabled())


def classifier_multilabel_any(Z, Wc, bc, label_bits, mask, weight, live=None):
    """Classifier + masked sigmoid cross-entropy + micro-F1 (models/base_gattn.py:50-59,71-94) for any embedding
    width / class count; label_bits: ops.pack_label_bits of the (N, C) multi-hot labels.  Returns a MultiLabelResult
    (loss, micro_f1, logits; .counts = [tp, fp, fn]).  live: as classifier_loss_any."""
    d = Z.shape[1]
    dm = _pad_to(d)
    if live is not None:
        return MultiLabelResult(*MultiLabelClassifierLoss.apply(Z, Wc, bc, label_bits, mask, weight,
                                                                torch.is_grad_enabled(), live))
    if dm != d:
        Z, Wc = torch.nn.functional.pad(Z, (0, dm - d)), torch.nn.functional.pad(Wc, (0, 0, 0, dm - d))
    return MultiLabelResult(*MultiLabelClassifierLoss.apply(Z, Wc, bc, label_bits, mask, weight, torch.is_grad_enabled()))


# ---------------------------------------------------------------------------
# reference-named functional API
# ---------------------------------------------------------------------------
def _squeeze_batch(seq, name="seq"):
    """The (N,F) features of a `seq` argument: a dense (1,N,F) / (N,F) tensor, or sparse features -- a SparseFeatures
    as it is, a torch sparse COO / CSR tensor (N,F) / (1,N,F) converted once (features.as_features)."""
    seq = as_features(seq)
    if isinstance(seq, SparseFeatures):
        return seq
    if seq.dim() == 3:
        if seq.shape[0] != 1:
            raise ValueError(f"{name}: batch size must be 1 (ex_acm3025.py:21; "
                             "utils/layers.py:110-113)")
        return seq[0]
    if seq.dim() != 2:
        raise ValueError(f"{name}: expected (1,N,F) or (N,F), got {tuple(seq.shape)}")
    return seq


def _single_head(seq, out_sz, graph, activation, in_drop, coef_drop, residual, params, training,
                 seed, return_coef=False):
    """One head of width out_sz.  Up to 64 columns it runs through the D=64 kernels (NodeLevelAttention): the head
    occupies slot 0 of K = 64/F'k head slots of the lane-mapped width F'k = next of 4, 8, 16, 32, 64 >= out_sz.
    Wider, it runs as ceil(out_sz / 64) column slices that share the head's scores, coefficients and per-head
    dropout draws (WideHeadAttention).  The columns beyond out_sz and the other slots have zero weights."""
    x = _squeeze_batch(seq)
    if out_sz < 1:
        raise ValueError("out_sz must be positive")
    Fin = x.shape[1]
    if params["W"].shape[0] != Fin:
        raise ValueError(f"W has {params['W'].shape[0]} input features, seq has {Fin}")
    wide = out_sz > D
    width = D * -(-out_sz // D)      # padded width of the head's columns

    def pad_last(t, w=width):
        out = t.new_zeros(t.shape[:-1] + (w,))
        out[..., :t.shape[-1]] = t
        return out

    W = pad_last(params["W"])[None]                                      # (1,F,width)
    if wide:
        a1, a2 = pad_last(params["a1"])[None], pad_last(params["a2"])[None]
        b1, b2 = params["b1"].reshape(1), params["b2"].reshape(1)
    else:
        fpk = next(w for w in (4, 8, 16, 32, 64) if out_sz <= w)
        K = D // fpk
        zeros = (params["W"] if isinstance(x, SparseFeatures) else x).new_zeros(K - 1, fpk)
        a1 = torch.cat([pad_last(params["a1"], fpk)[None], zeros])[None]   # (1,K,F'k)
        a2 = torch.cat([pad_last(params["a2"], fpk)[None], zeros])[None]
        b1 = pad_last(params["b1"].reshape(1), K)[None]
        b2 = pad_last(params["b2"].reshape(1), K)[None]
    c = pad_last(params["c"])[None]
    code, post = _act_code(activation)
    train = bool(training) or in_drop > 0 or coef_drop > 0 or W.requires_grad
    run = LayerRun(train=train, in_drop=in_drop, coef_drop=coef_drop,
                   seeds=(rng.next_seed() if seed is None else seed,), act=code,
                   coef_sink=[] if return_coef else None, coef_mean=wide)
    Wr = br = None
    if residual and Fin != out_sz:
        # utils/layers.py:38-40: + conv1d(seq, out_sz, 1) of the DROPPED input, before the
        # activation; when the widths are equal the reference's branch is a no-op (:42)
        Wr, br = pad_last(params["res_W"])[None], pad_last(params["res_b"])[None]
    fn = WideHeadAttention if wide else NodeLevelAttention
    M = fn.apply(None, W, a1, b1, a2, b2, c, Wr, br, (x,), (graph,), run)
    ret = M[:, 0, :out_sz]
    if post is not None:
        ret = post(ret)
    if return_coef:       # the head's mean over its one head (wide), or slot 0 of the K head slots
        coef = run.coef_sink[0] if wide else run.coef_sink[0][:, 0]
        coefs = torch.sparse_csr_tensor(graph.rowptr, graph.colidx.long(), coef.contiguous(),
                                        (graph.n_rows, graph.n_cols))
        return ret[None], coefs
    return ret[None]     # (1,N,out_sz)


def attn_head(seq, out_sz, bias_mat, activation, in_drop=0.0, coef_drop=0.0, residual=False,
              return_coef=False, *, params, training=False, seed=None):
    """utils/layers.py:7-46.  seq (1,N,F); bias_mat (1,N,N) additive mask, or a
    CSRGraph / (rowptr, colidx) pair.  params: dict W (F,out_sz), a1 (out_sz,),
    b1 (), a2 (out_sz,), b2 (), c (out_sz,) [+ res_W (F,out_sz), res_b (out_sz,) when
    residual=True and F != out_sz].
    return_coef=True also returns `coefs` (:43-44) -- the (dropped) softmax weights --
    as a torch sparse CSR tensor (N,N) over the stored neighbours (every masked entry
    of the reference's dense (1,N,N) tensor is exactly 0: exp(-1e9) == 0 in fp32);
    data only, no gradient flows through it."""
    return _single_head(seq, out_sz, as_graph(bias_mat, seq.device), activation, in_drop,
                        coef_drop, residual, params, training, seed, return_coef=return_coef)


def attn_head_const_1(seq, out_sz, bias_mat, activation, in_drop=0.0, coef_drop=0.0, residual=False, *,
                      params, training=False, seed=None):
    """utils/layers.py:49-81 (the HAN_nd ablation): logits := adjacency, i.e. every
    stored neighbour gets the same weight 1/deg (mean aggregator).  The same kernel
    with zero score parameters.  params: W (F,out_sz), c (out_sz,)."""
    z = torch.zeros_like(params["c"])
    p = {"W": params["W"], "a1": z, "a2": z, "b1": z.new_zeros(()), "b2": z.new_zeros(()), "c": params["c"]}
    for k in ("res_W", "res_b"):
        if k in params:
            p[k] = params[k]
    return attn_head(seq, out_sz, bias_mat, activation, in_drop=in_drop, coef_drop=coef_drop,
                     residual=residual, params=p, training=training, seed=seed)


def sp_attn_head(seq, out_sz, adj_mat, activation, nb_nodes, in_drop=0.0, coef_drop=0.0,
                 residual=False, *, params, training=False, seed=None):
    """utils/layers.py:85-127.  adj_mat: torch sparse (1,N,N)/(N,N) tensor, a
    CSRGraph or (rowptr, colidx).  Stored values other than 1 scale the logits,
    e_ij = LeakyReLU(v_ij*f1_i + v_ij*f2_j) (:95-98), as in the reference -- they
    are not a mask; the softmax runs over the stored entries (:100)."""
    g = as_graph(adj_mat, seq.device)
    if g.n_rows != nb_nodes:
        raise ValueError(f"nb_nodes={nb_nodes} but adj_mat has {g.n_rows} rows")
    return _single_head(seq, out_sz, g, activation, in_drop, coef_drop, residual, params, training,
                        seed)


def SimpleAttLayer(inputs, attention_size, time_major=False, return_alphas=False, *, params, semantic="node"):
    """utils/layers.py:132-164.  inputs (N,P,D) [or (P,N,D) if time_major, or a
    tuple to be concatenated on the last axis]; params: w_omega (D,A),
    b_omega (A,), u_omega (A,).  semantic="metapath": one weight per meta-path (han.pdf eq. 7-9)."""
    if isinstance(inputs, tuple):
        inputs = torch.cat(inputs, 2)                    # :134-136
    if time_major:
        inputs = inputs.transpose(0, 1)                  # :138-140
    if params["w_omega"].shape != (inputs.shape[2], attention_size):
        raise ValueError("w_omega must be (hidden_size, attention_size)")
    out, alphas = semantic_attention(inputs.contiguous(), params["w_omega"], params["b_omega"],
                                     params["u_omega"], mode=semantic)
    if not return_alphas:
        return out
    return out, alphas
