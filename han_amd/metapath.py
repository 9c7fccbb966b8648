"""Meta-path graphs from typed relations (K0): the inputs of ``HeteGAT_multi.inference``.

The reference reads its meta-path graphs preprocessed (``ex_acm3025.py:57-87``: PAP, PLP, ... as dense matrices of a
``.mat`` file) and leaves building them to the user.  Here a meta-path such as APCPA is the boolean product of the
typed relations along it -- paper-author, paper-conference, ... edge lists --, computed on the GPU by
``ops.csr_bool_matmul`` (``han_spgemm_*``, ``csrc/metapath.hip``).  With ``weights="count"`` / ``"pathsim"`` the
product is taken over the integers (``ops.csr_count_matmul``) and the graph carries the instance counts or their
PathSim as ``values``; ``top_k`` keeps the strongest neighbours of every node.  The results are ``CSRGraph``s that go
straight into ``bias_mat_list``::

    rel = {"AP": relation(author_ids, paper_ids, n_authors, n_papers, device=dev),
           "PC": relation(paper_ids2, conf_ids, n_papers, n_confs, device=dev)}
    graphs = [metapath_graph(rel, mp) for mp in ("APA", "APCPA")]

Where a hub type sits on the path (a conference, a term) the product is close to dense, and ``top_k`` prunes a graph
that first has to exist.  ``metapath_sample`` draws the neighbours instead: meta-path-guided random walks from every
node, the ``fanout`` most visited end points kept (``ops.metapath_walk``, ``han_metapath_walk_*``)::

    graphs = [metapath_sample(rel, mp, walks=256, fanout=32, weights="prob") for mp in ("APCPA", "APTPA")]

Node types are single letters; ``relations`` maps an ordered pair ``"XY"`` to the graph with rows = X nodes and
columns = Y nodes, and a hop Y -> X without its own relation runs on the transpose of ``"XY"``.
"""
from __future__ import annotations

import numpy as np
import torch

from . import csr, ops
from .graph import CSRGraph


def _ids(x, name, device):
    t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
    if t.dim() != 1:
        raise ValueError(f"{name}: expected a 1-D array of node ids, got shape {tuple(t.shape)}")
    if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
        raise ValueError(f"{name}: integer node ids expected, got {t.dtype}")
    if device is not None:
        t = t.to(device)
    return t.to(torch.int64)


def _from_keys(key, n_rows, n_cols) -> CSRGraph:
    """CSR of the sorted, unique entry keys row * n_cols + col."""
    rowptr, cols = csr.from_sorted_keys(key, n_rows, n_cols)
    return CSRGraph(rowptr, cols.to(torch.int32), n_cols, validate=False)


def relation(src, dst, n_src: int, n_dst: int, device=None) -> CSRGraph:
    """The graph of one typed relation from its edge list: rows = `src` nodes (n_src of them), columns = `dst` nodes,
    columns sorted and repeated edges dropped.  src / dst: numpy or torch integer arrays of equal length; the graph
    lives on `device` (default: where `src` is).  Raises ValueError on ids outside [0, n_src) / [0, n_dst)."""
    n_src, n_dst = int(n_src), int(n_dst)
    if n_src < 0 or n_dst < 0 or n_dst > 2 ** 31 - 1:
        raise ValueError(f"sizes {n_src} x {n_dst}: expected n_src >= 0 and 0 <= n_dst < 2^31 (int32 columns)")
    s = _ids(src, "src", device)
    d = _ids(dst, "dst", s.device)
    if s.shape != d.shape:
        raise ValueError(f"src has {s.numel()} ids, dst {d.numel()}")
    if s.numel():
        for t, n, name in ((s, n_src, "src"), (d, n_dst, "dst")):
            lo, hi = int(t.min()), int(t.max())
            if lo < 0 or hi >= n:
                raise ValueError(f"{name} ids outside [0, {n}): [{lo}, {hi}]")
    return _from_keys(torch.unique(s * n_dst + d), n_src, n_dst)


WEIGHTS = (None, "count", "pathsim")


def _check_weights(weights, top_k=None):
    if weights not in WEIGHTS:
        raise ValueError(f"weights = {weights!r}: expected None, 'count' or 'pathsim'")
    if top_k is not None:
        if weights is None:
            raise ValueError("top_k needs weights ('count' or 'pathsim'): a boolean graph has nothing to rank")
        if isinstance(top_k, bool) or int(top_k) != top_k or top_k < 1:
            raise ValueError(f"top_k = {top_k!r}: expected an integer >= 1")


def _weighted(g: CSRGraph, counts, weights, top_k=None) -> CSRGraph:
    """`g` with the values that `weights` asks for from its instance counts, cut to top_k entries per row."""
    values = counts.to(torch.float32) if weights == "count" else ops.csr_pathsim(g, counts)
    g = CSRGraph(g.rowptr, g.colidx, g.n_cols, validate=False, values=values)
    return g if top_k is None else ops.csr_row_topk(g, int(top_k), keep_diag=True)


def _check_chain(graphs, self_loops):
    if not graphs:
        raise ValueError("compose: no graphs")
    for k, g in enumerate(graphs):
        if not isinstance(g, CSRGraph):
            raise ValueError(f"compose: graphs[{k}] is a {type(g)}, expected a CSRGraph")
    for k in range(len(graphs) - 1):
        if graphs[k].n_cols != graphs[k + 1].n_rows:
            raise ValueError(f"compose: graphs[{k}] has {graphs[k].n_cols} columns, graphs[{k + 1}] has "
                             f"{graphs[k + 1].n_rows} rows")
    if self_loops and graphs[0].n_rows != graphs[-1].n_cols:
        raise ValueError(f"compose: self_loops needs a square result, got {graphs[0].n_rows} x {graphs[-1].n_cols}")


def _compose(graphs, self_loops, counted):
    """(graph, counts) of the chain left to right; counts None unless `counted` (then int64 per entry: the instances,
    every product fed the counts of the one before as operand values)."""
    if len(graphs) == 1:       # no product: the graph itself, sorted and unique (+ I)
        g = graphs[0]
        key = csr.row_ids(g.rowptr) * g.n_cols + g.colidx.long()
        n_stored = key.numel()
        if self_loops:
            key = torch.cat([key, torch.arange(g.n_rows, device=g.device) * (g.n_cols + 1)])
        if not counted:
            return _from_keys(torch.unique(key), g.n_rows, g.n_cols), None
        key, inv = torch.unique(key, return_inverse=True)
        counts = torch.bincount(inv[:n_stored], minlength=key.numel())      # an added (i, i) counts 0
        return _from_keys(key, g.n_rows, g.n_cols), counts
    c, counts = graphs[0], None
    for k, g in enumerate(graphs[1:]):
        diag = self_loops and k == len(graphs) - 2
        if counted:
            c, counts = ops.csr_count_matmul(c, g, a_counts=counts, diag=diag)
        else:
            c = ops.csr_bool_matmul(c, g, diag=diag)
    return c, counts


def compose(graphs, self_loops: bool = False, weights=None) -> CSRGraph:
    """The product of a chain of graphs, left to right: entry (i, j) iff a path i -> ... -> j exists
    (graphs[k].n_cols == graphs[k+1].n_rows).  self_loops=True needs a square result and adds (i, i).  The result
    has strictly increasing columns per row.  weights=None: the boolean product, values None.  weights="count": values
    = the number of paths i -> ... -> j as fp32 (a repeated stored entry of a graph is as many parallel edges), 0 for an
    (i, i) that only self_loops added.  weights="pathsim" (square results): values = 2 c_ij / (c_ii + c_jj), 1 on the
    diagonal.  GPU graphs only (han_amd has no CPU path)."""
    graphs = list(graphs)
    _check_weights(weights)
    _check_chain(graphs, self_loops)
    if weights == "pathsim" and graphs[0].n_rows != graphs[-1].n_cols:
        raise ValueError(f"compose: weights='pathsim' needs a square result, got {graphs[0].n_rows} x "
                         f"{graphs[-1].n_cols}")
    for k, g in enumerate(graphs):
        ops.require_gpu(g.rowptr, f"compose: graphs[{k}]")
    c, counts = _compose(graphs, self_loops, weights is not None)
    return c if weights is None else _weighted(c, counts, weights)


def plan(relations: dict, metapath: str) -> dict:
    """How `metapath` is evaluated (host only, no graph is touched): dict(hops=[(pair, transposed)] -- one per hop,
    the relation it uses and whether that is the transpose of the reverse pair --, split = k or None, sizes = nodes per
    type).  split = k: the path is a palindrome of odd length whose second half is made only of derived transposes,
    so it equals H Hᵀ with H the product of its first k hops.  Raises ValueError for a pair given in both
    directions, a missing pair, type sizes that disagree between relations, or malformed keys / paths."""
    if not isinstance(metapath, str) or len(metapath) < 2:
        raise ValueError(f"meta-path {metapath!r}: expected a string of at least two one-letter node types")
    sizes = {}
    for key, g in relations.items():
        if not (isinstance(key, str) and len(key) == 2):
            raise ValueError(f"relation key {key!r}: expected an ordered pair of one-letter node types such as 'PA'")
        if not isinstance(g, CSRGraph):
            raise ValueError(f"relations[{key!r}] is a {type(g)}, expected a CSRGraph (see relation())")
        if key[0] != key[1] and key[::-1] in relations:
            raise ValueError(f"relation {key!r} is given in both directions ({key!r} and {key[::-1]!r}): give one, "
                             "the other hop runs on its transpose")
        for t, n in ((key[0], g.n_rows), (key[1], g.n_cols)):
            if sizes.setdefault(t, n) != n:
                raise ValueError(f"type {t!r} has {sizes[t]} nodes in one relation and {n} in {key!r}")
    hops = []
    for x, y in zip(metapath, metapath[1:]):
        if x + y in relations:
            hops.append((x + y, False))
        elif y + x in relations:
            hops.append((y + x, True))
        else:
            raise ValueError(f"meta-path {metapath!r}: no relation between {x!r} and {y!r} (give {x + y!r} or {y + x!r})")
    split = None
    if len(metapath) % 2 == 1 and metapath == metapath[::-1] and all(t for _, t in hops[len(hops) // 2:]):
        split = len(hops) // 2
    return dict(hops=hops, split=split, sizes=sizes)


def _transposed(g: CSRGraph, counts):
    """(gᵀ, its counts): the int64 counts ride through the sort that builds gᵀ (its fp32 values would round them)."""
    return g.transpose_with(counts)


def metapath_graph(relations: dict, metapath: str, self_loops: bool = True, weights=None, top_k=None) -> CSRGraph:
    """The meta-path graph of `metapath` (e.g. "APCPA") over typed `relations` ({"AP": CSRGraph, "PC": ...}):
    entry (i, j) iff an instance of the path leads from i to j; with self_loops (the default, as adj_to_bias /
    adj_to_graph add I) also (i, i).  A palindromic path whose second half runs on derived transposes is evaluated as
    H Hᵀ, H = the product over its first half (AP PC for APCPA, AP for APA) -- the same graph as the chain left to
    right, without the chain's wide intermediates; any other path left to right (compose).

    weights: None -- a boolean graph (values None); "count" -- values = the number of path instances between i and j,
    as fp32 (exact below 2^24); "pathsim" -- values = 2 c_ij / (c_ii + c_jj) in (0, 1], the form meant for training
    (metapath must read the same backwards).  An (i, i) that only self_loops added has count 0 and PathSim 1.  The
    values scale the attention logits (CSRGraph.values), so raw counts saturate the softmax.  top_k (needs weights):
    keep per row the top_k strongest neighbours besides (i, i), ties to the smaller column (ops.csr_row_topk).  H is
    built with counts and enters H Hᵀ as operand values, so both plans count the same instances."""
    _check_weights(weights, top_k)
    p = plan(relations, metapath)
    if self_loops and metapath[0] != metapath[-1]:
        raise ValueError(f"meta-path {metapath!r}: self_loops needs a path that ends on the type it starts from")
    if weights == "pathsim" and metapath != metapath[::-1]:
        raise ValueError(f"meta-path {metapath!r}: weights='pathsim' needs a path that reads the same backwards")
    for key, _ in p["hops"]:
        ops.require_gpu(relations[key].rowptr, f"relations[{key!r}]")
    graphs = [relations[k].transpose() if t else relations[k] for k, t in p["hops"]]
    counted = weights is not None
    if p["split"] is None:
        _check_chain(graphs, self_loops)
        g, counts = _compose(graphs, self_loops, counted)
    else:
        k = p["split"]
        h, hc = _compose(graphs[:k], False, counted) if k > 1 else (graphs[0], None)
        if not counted:
            return ops.csr_bool_matmul(h, h.transpose(), diag=self_loops)
        ht, htc = _transposed(h, hc) if hc is not None else (h.transpose(), None)
        g, counts = ops.csr_count_matmul(h, ht, a_counts=hc, b_counts=htc, diag=self_loops)
    return g if not counted else _weighted(g, counts, weights, top_k)


SAMPLE_WEIGHTS = (None, "count", "prob")


def metapath_sample(relations: dict, metapath: str, walks: int = 256, fanout=32, seed: int = 0,
                    self_loops: bool = True, weights=None, rows=None) -> CSRGraph:
    """Sampled neighbours of `metapath` over typed `relations`, without the product: from every start node `walks`
    random walks along the path -- at every hop a uniformly drawn stored entry of the current node's row, a reverse hop
    on the transpose as in metapath_graph; a node without entries ends the walk --, and per start node the `fanout`
    (None = walks) most visited end points, ties to the smaller id.  Every entry is an entry of metapath_graph(...);
    a row holds at most fanout + 1.  self_loops (the default; the path must end on the type it starts from): (i, i) is
    always stored, with its own visit count, and does not compete for fanout.

    weights: None -- a boolean graph; "count" -- values = the visits c_ij as fp32; "prob" -- c_ij / walks in fp32, the
    estimate of the random-walk transition probability (walks that died stay in the denominator): in [0, 1], like
    PathSim it does not saturate the softmax.  An (i, i) that no walk reached has value 0.
    seed: 64 bits; the draw of (start node, walk, hop) is a counter-based hash of it (include/han_hip.h), so the result
    is bitwise reproducible and rows = (r0, r1) returns exactly those rows of the whole graph, with global columns and
    row_base = r0 -- the shard a rank hands to HANTrainer(graphs_local=True).  The H Hᵀ form of metapath_graph is
    never used: a walk has no use for H."""
    if weights not in SAMPLE_WEIGHTS:
        raise ValueError(f"weights = {weights!r}: expected None, 'count' or 'prob'")
    walks, fanout, seed = ops._walk_limits(walks, fanout, seed)
    p = plan(relations, metapath)
    if len(p["hops"]) > ops.WALK_MAX_HOPS:
        raise ValueError(f"meta-path {metapath!r}: {len(p['hops'])} hops, at most {ops.WALK_MAX_HOPS} are walked")
    if self_loops and metapath[0] != metapath[-1]:
        raise ValueError(f"meta-path {metapath!r}: self_loops needs a path that ends on the type it starts from")
    ops._walk_rows(rows, p["sizes"][metapath[0]])
    for key, _ in p["hops"]:
        ops.require_gpu(relations[key].rowptr, f"relations[{key!r}]")
    hops = [relations[k].transpose() if t else relations[k] for k, t in p["hops"]]
    g, visits = ops.metapath_walk(hops, walks, fanout, seed=seed, diag=self_loops, rows=rows)
    if weights is None:
        return g
    values = visits.to(torch.float32)
    if weights == "prob":
        values = values / torch.tensor(float(walks), dtype=torch.float32, device=values.device)
    return CSRGraph(g.rowptr, g.colidx, g.n_cols, validate=False, values=values, row_base=g.row_base)
