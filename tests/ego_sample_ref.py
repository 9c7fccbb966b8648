"""NumPy reference of the sampled ego-block rule (han_amd/minibatch.py: ego_block(..., fanout=, seed=)).

Graphs are the (rowptr, colidx, values) triples of tests/ego_block_ref.py.  The key of the entry at stored position k
of row v of graph number p is the first word of han_rand64(seed, 4 (p + 1), v, k) (tests/rng_ref.py); a row closer
than `hops` keeps its self entries and, of its d other entries, all when d <= fanout[level], else the fanout[level]
of smallest (key, k).
"""
import numpy as np

from tests import ego_block_ref as ref
from tests.rng_ref import han_rand64

_M64 = (1 << 64) - 1


def row_keys(seed, p, v, d):
    """(d,) uint64 holding the 32-bit keys of the stored positions 0 .. d - 1 of row v of graph p."""
    x, _ = han_rand64(int(seed) & _M64, 4 * (p + 1), np.uint64(v), np.arange(d, dtype=np.uint64))
    return x


def select_positions(cols, v, p, f, seed):
    """Ascending stored positions of the entries row v (columns `cols`) of graph p keeps at fan-out f."""
    cols = np.asarray(cols)
    k = np.arange(cols.size)
    other = k[cols != v]
    if other.size <= f:
        return k
    x = row_keys(seed, p, v, cols.size)[other]
    keep = cols == v
    keep[other[np.lexsort((other, x))[:f]]] = True           # smallest key first, equal keys by stored position
    return k[keep]


def fanouts(fanout, hops):
    return [int(fanout)] * hops if np.ndim(fanout) == 0 else [int(f) for f in fanout]


def sampled_rows(graphs, seeds, hops, fanout, seed):
    """(level (n,) int32, sel): breadth-first levels over the union of the sampled rows and, per graph, the dict
    row -> kept positions of every row with level < hops."""
    fan = fanouts(fanout, hops)
    assert len(fan) == hops
    n = graphs[0][0].size - 1
    level = np.full(n, -1, dtype=np.int32)
    level[np.asarray(seeds, dtype=np.int64)] = 0
    sel = [dict() for _ in graphs]
    for h in range(hops):
        frontier = np.nonzero(level == h)[0]
        for p, (rowptr, colidx, _) in enumerate(graphs):
            for i in frontier:
                row = colidx[rowptr[i]:rowptr[i + 1]]
                sel[p][int(i)] = pos = select_positions(row, i, p, fan[h], seed)
                cols = row[pos]
                level[cols[level[cols] < 0]] = h + 1
    return level, sel


def thinned(graphs, sel):
    """G': the graphs with every row of sel replaced by its selected entries, every other row as it is."""
    out = []
    for (rowptr, colidx, values), s in zip(graphs, sel):
        rows, vals = [], []
        for i in range(rowptr.size - 1):
            e = np.arange(rowptr[i], rowptr[i + 1])
            if i in s:
                e = e[s[i]]
            rows.append(colidx[e])
            vals.append(values[e] if values is not None else None)
        out.append(ref.from_rows(rows, vals if values is not None else None))
    return out


def thinned_graphs(graphs, seeds, hops, fanout, seed):
    return thinned(graphs, sampled_rows(graphs, seeds, hops, fanout, seed)[1])


def ego_sample_ref(graphs, seeds, hops, fanout, seed):
    """The sampled block, built directly from the selection (the layout of ego_block_ref's result)."""
    level, sel = sampled_rows(graphs, seeds, hops, fanout, seed)
    nodes = np.nonzero(level >= 0)[0].astype(np.int64)
    local = np.full(level.size, -1, dtype=np.int32)
    local[nodes] = np.arange(nodes.size, dtype=np.int32)
    out = []
    for (rowptr, colidx, values), s in zip(graphs, sel):
        rows, vals = [], []
        for r, v in enumerate(nodes):
            if level[v] < hops:
                e = rowptr[v] + s[int(v)]
                rows.append(local[colidx[e]])
                vals.append(values[e] if values is not None else None)
            else:
                rows.append(np.array([r], dtype=np.int32))
                vals.append(np.ones(1, dtype=np.float32))
        out.append(ref.from_rows(rows, vals if values is not None else None))
    return dict(nodes=nodes, level=level[nodes], seed_pos=local[np.asarray(seeds, dtype=np.int64)].astype(np.int64),
                graphs=out)


def blocks_equal(a, b):
    same = all(np.array_equal(a[k], b[k]) and a[k].dtype == b[k].dtype for k in ("nodes", "level", "seed_pos"))
    for (rp, ci, va), (rq, cj, vb) in zip(a["graphs"], b["graphs"]):
        same = same and np.array_equal(rp, rq) and np.array_equal(ci, cj) and (va is None) == (vb is None)
        same = same and (va is None or np.array_equal(va, vb))
    return same and len(a["graphs"]) == len(b["graphs"])


def tie_fanout(seed, p, v, d):
    """(f, pairs): a fan-out at which the f-th and (f + 1)-th smallest (key, position) of a row of d entries off the
    diagonal share their key -- the first such --, and the number of adjacent equal keys in sorted order."""
    x = np.sort(row_keys(seed, p, v, d))
    eq = np.nonzero(x[1:] == x[:-1])[0]
    return (int(eq[0]) + 1 if eq.size else None), int(eq.size)
