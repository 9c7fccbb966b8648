"""NumPy reference of the ego-block rule (han_amd/minibatch.py), and a brute-force check of its node set.

A graph is (rowptr int64 (n + 1,), colidx int32 (nnz,), values float32 (nnz,) or None).  Row i points at its
columns: the neighbours whose rows feed row i.
"""
import numpy as np


def from_rows(rows, values=None):
    """(rowptr, colidx, values) of a list of per-row column lists, stored order and repeats kept; values: None or a
    list of per-row value lists."""
    rowptr = np.zeros(len(rows) + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum([len(r) for r in rows])
    colidx = np.concatenate([np.asarray(r, dtype=np.int32) for r in rows]) if rowptr[-1] else np.zeros(0, np.int32)
    vals = None
    if values is not None:
        vals = np.concatenate([np.asarray(v, dtype=np.float32) for v in values]) if rowptr[-1] else np.zeros(0, np.float32)
    return rowptr, colidx.astype(np.int32), vals


def ego_block_ref(graphs, seeds, hops):
    """dict(nodes int64 ascending, level int32, seed_pos int64, graphs [(rowptr, colidx, values)]): breadth-first
    levels over the union of the graphs, rows with level < hops kept whole, rim rows (level == hops) hold (r, r)."""
    n = graphs[0][0].size - 1
    seeds = np.asarray(seeds, dtype=np.int64)
    level = np.full(n, -1, dtype=np.int32)
    level[seeds] = 0
    for h in range(hops):
        frontier = np.nonzero(level == h)[0]
        for rowptr, colidx, _ in graphs:
            for i in frontier:
                cols = colidx[rowptr[i]:rowptr[i + 1]]
                level[cols[level[cols] < 0]] = h + 1
    nodes = np.nonzero(level >= 0)[0].astype(np.int64)
    local = np.full(n, -1, dtype=np.int32)
    local[nodes] = np.arange(nodes.size, dtype=np.int32)
    out = []
    for rowptr, colidx, values in graphs:
        rows, vals = [], []
        for r, v in enumerate(nodes):
            if level[v] < hops:
                rows.append(local[colidx[rowptr[v]:rowptr[v + 1]]])
                vals.append(values[rowptr[v]:rowptr[v + 1]] if values is not None else None)
            else:
                rows.append(np.array([r], dtype=np.int32))
                vals.append(np.ones(1, dtype=np.float32))
        out.append(from_rows(rows, vals if values is not None else None))
    return dict(nodes=nodes, level=level[nodes], seed_pos=local[seeds].astype(np.int64), graphs=out)


def brute_force_levels(graphs, seeds, hops):
    """(n,) distance from the seed set by dense powers of U = A_1 | ... | A_P | I: the smallest k <= hops with
    (U^k)[seed, v] set for some seed, -1 when there is none."""
    n = graphs[0][0].size - 1
    u = np.eye(n, dtype=bool)
    for rowptr, colidx, _ in graphs:
        rows = np.repeat(np.arange(n), np.diff(rowptr))
        u[rows, colidx] = True
    level = np.full(n, -1, dtype=np.int32)
    reach = np.zeros(n, dtype=bool)
    reach[np.asarray(seeds)] = True                      # U^0
    level[reach] = 0
    for k in range(1, hops + 1):
        reach = (reach[:, None] & u).any(0)             # the rows of U^k summed over the seeds
        level[reach & (level < 0)] = k
    return level
