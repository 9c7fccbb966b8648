"""The host-side CSR helpers (han_amd/csr.py) against plain-Python loops, on the CPU, at the smallest shapes where each
can go wrong; and CSRGraph.transpose_with / metapath._transposed on a graph with repeated entries."""
import pytest
import torch

from han_amd import csr, metapath
from han_amd.graph import CSRGraph

I64 = torch.int64


def _t(xs, dtype=I64):
    return torch.tensor(xs, dtype=dtype)


COUNTS = [[], [0, 0, 0], [5], [0, 3, 0, 2, 0], [2, 1, 4]]


@pytest.mark.parametrize("counts", COUNTS)
def test_scan_and_row_ids(counts):
    ptr = csr.scan(_t(counts))
    want = [0]
    for c in counts:
        want.append(want[-1] + c)
    assert ptr.dtype == I64 and ptr.tolist() == want
    ids = [i for i, c in enumerate(counts) for _ in range(c)]
    got = csr.row_ids(ptr)
    assert got.dtype == I64 and got.tolist() == ids
    got = csr.row_ids(ptr, torch.int32, base=7)
    assert got.dtype == torch.int32 and got.tolist() == [7 + i for i in ids]


def test_scan_takes_narrow_counts():
    assert csr.scan(_t([1, 2], torch.int32)).dtype == I64


@pytest.mark.parametrize("keys,n_groups", [([], 3), ([1, 2, 1], 4), ([2, 2, 2], 3), ([3, 0, 3, 1, 0, 3, 1], 4),
                                           ([0, 0, 0, 0], 1), ([], 0)])
def test_group_by(keys, n_groups):
    """no keys; no member in the first and last group; every key equal; repeated keys; one group."""
    ptr, order = csr.group_by(_t(keys), n_groups)
    groups = [[e for e, k in enumerate(keys) if k == grp] for grp in range(n_groups)]     # input order inside a group
    assert ptr.dtype == I64 and order.dtype == I64
    assert ptr.tolist() == [sum(len(g) for g in groups[:k]) for k in range(n_groups + 1)]
    assert order.tolist() == [e for g in groups for e in g]


LENS = [0, 4, 5, 8, 9, 12, 13]


@pytest.mark.parametrize("longer_than,chunk", [(8, 4), (4, 4)])
def test_chunk_table(longer_than, chunk):
    ptr = csr.scan(_t(LENS))
    t = csr.chunk_table(ptr, longer_than, chunk)
    long = [s for s, n in enumerate(LENS) if n > longer_than]
    assert LENS.index(longer_than) not in long and LENS.index(longer_than + 1) in long
    assert t["n_long"] == len(long) and t["long"].tolist() == long
    chunks = []                                     # (index into long, start, end), segment after segment, in order
    for k, s in enumerate(long):
        for b in range(int(ptr[s]), int(ptr[s + 1]), chunk):
            chunks.append((k, b, min(b + chunk, int(ptr[s + 1]))))
    assert t["n_chunks"] == len(chunks)
    assert t["chunk_long"].tolist() == [c[0] for c in chunks]
    assert t["chunk_start"].tolist() == [c[1] for c in chunks]
    assert t["chunk_end"].tolist() == [c[2] for c in chunks]
    assert t["long_ptr"].tolist() == [sum(1 for c in chunks if c[0] < k) for k in range(len(long) + 1)]
    for name in ("long", "long_ptr", "chunk_long", "chunk_start", "chunk_end"):
        assert t[name].dtype == I64 and t[name].is_contiguous(), name
    # the chunks of a segment tile it exactly, none is empty (12 = 3 x 4 has three chunks, not four)
    for k, s in enumerate(long):
        mine = [(b, e) for kk, b, e in chunks if kk == k]
        got = [(int(b), int(e)) for kk, b, e in zip(t["chunk_long"], t["chunk_start"], t["chunk_end"]) if kk == k]
        assert got == mine and got[0][0] == int(ptr[s]) and got[-1][1] == int(ptr[s + 1])
        assert all(0 < e - b <= chunk for b, e in got) and all(a[1] == b[0] for a, b in zip(got, got[1:]))
        assert len(got) == -(-LENS[s] // chunk)


def test_chunk_table_none_when_nothing_is_long():
    assert csr.chunk_table(csr.scan(_t(LENS)), 13, 4) is None
    assert csr.chunk_table(csr.scan(_t([])), 0, 4) is None
    assert csr.chunk_table(csr.scan(_t([0, 0])), 0, 4) is None


@pytest.mark.parametrize("starts,lens", [([], []), ([5, 0, 9], [0, 0, 0]), ([7, 3, 3, 20, 0], [2, 0, 3, 1, 0]),
                                         ([4], [3])])
def test_ragged_index(starts, lens):
    got = csr.ragged_index(_t(starts), _t(lens))
    assert got.dtype == I64 and got.tolist() == [s + k for s, n in zip(starts, lens) for k in range(n)]


@pytest.mark.parametrize("entries,n_rows,n_cols", [([], 3, 4), ([], 0, 0), ([(1, 0), (1, 3), (2, 2)], 5, 4),
                                                   ([(0, 0), (0, 1), (3, 1)], 4, 2)])
def test_from_sorted_keys(entries, n_rows, n_cols):
    """no entry (also of a 0 x 0 matrix); empty rows at both ends; rows filled to the last column."""
    rowptr, cols = csr.from_sorted_keys(_t([r * n_cols + c for r, c in entries]), n_rows, n_cols)
    assert rowptr.dtype == I64 and cols.dtype == I64
    assert rowptr.tolist() == [sum(1 for r, _ in entries if r < i) for i in range(n_rows + 1)]
    assert cols.tolist() == [c for _, c in entries]


@pytest.mark.parametrize("counts", [[], [0, 0, 0], [2, 0, 3]])
def test_two_pass(counts):
    calls = []

    def count(out):
        assert out.shape == (len(counts),) and out.dtype == I64
        calls.append("count")
        out.copy_(_t(counts))

    def fill(rowptr, cols, vals):
        calls.append("fill")
        assert int(rowptr[-1]) == sum(counts)
        cols.copy_(torch.arange(sum(counts)))
        vals.fill_(0.5)

    rowptr, cols, vals = csr.two_pass(len(counts), torch.device("cpu"), (torch.int32, torch.float32), count, fill)
    assert rowptr.dtype == I64 and rowptr.tolist() == [sum(counts[:i]) for i in range(len(counts) + 1)]
    assert cols.dtype == torch.int32 and vals.dtype == torch.float32 and cols.shape == vals.shape == (sum(counts),)
    if sum(counts):
        assert calls == ["count", "fill"] and cols.tolist() == list(range(sum(counts)))
        assert vals.tolist() == [0.5] * sum(counts)
    else:                                           # no entries: fill is not called; no rows: nothing is
        assert calls == (["count"] if counts else [])


def test_transpose_carries_per_entry_arrays():
    """A multigraph (repeated entries, unsorted columns, an empty row, an unused column): the carried int64 array
    follows its entries through the one sort, and metapath._transposed returns CSRGraph.transpose's graph."""
    rows = [[2, 0, 2], [], [4, 2, 2, 0], [1]]
    rowptr = csr.scan(_t([len(r) for r in rows]))
    colidx = _t([c for r in rows for c in r], torch.int32)
    counts = (torch.arange(colidx.numel()) + 1) * (1 << 40)        # beyond what fp32 values could carry
    vals = torch.arange(colidx.numel(), dtype=torch.float32) + 0.5
    # entries of column j in input order: (row, count, value)
    want = [[(i, int(counts[e]), float(vals[e])) for i in range(4) for e in range(int(rowptr[i]), int(rowptr[i + 1]))
             if int(colidx[e]) == j] for j in range(6)]
    flat = [x for col in want for x in col]

    def check(t, tc):
        assert (t.n_rows, t.n_cols) == (6, 4) and t.colidx.dtype == torch.int32 and tc.dtype == I64
        assert t.rowptr.tolist() == [sum(len(c) for c in want[:j]) for j in range(7)]
        assert t.colidx.tolist() == [x[0] for x in flat] and tc.tolist() == [x[1] for x in flat]
        assert t.values.tolist() == [x[2] for x in flat]

    g = CSRGraph(rowptr, colidx, 6, values=vals)
    t, tc = metapath._transposed(g, counts)                         # builds the transpose
    check(t, tc)
    assert g.transpose() is t and t.transpose() is g
    t2, tc2, tv2 = g.transpose_with(counts, vals)                  # beside the cached transpose
    assert t2 is t and torch.equal(tc2, tc) and torch.equal(tv2, t.values)
    plain = CSRGraph(rowptr, colidx, 6, values=vals).transpose()   # transpose alone builds the same graph
    assert torch.equal(plain.rowptr, t.rowptr) and torch.equal(plain.colidx, t.colidx)
    assert torch.equal(plain.values, t.values)
