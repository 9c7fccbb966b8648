"""han_amd.SparseFeatures on the host: constructors, canonical form, validation, the transposed image with its chunk
table, the bag-of-words generator and the partition guard.  No GPU is touched."""
import types

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from han_amd import SparseFeatures, ops, synth

N, F = 37, 53


def _entries():
    """COO triples of the 37 x 53 test matrix, in scrambled order: row 3 empty, row 5 full (but for the empty column),
    column 7 empty, the entry (2, 11) three times (summed), unsorted columns everywhere, a stored zero at (9, 4)."""
    rng = np.random.default_rng(5)
    rows, cols, vals = [], [], []
    for r in range(N):
        if r == 3:
            continue
        cs = np.arange(F) if r == 5 else rng.choice(F, size=rng.integers(1, 9), replace=False)
        for c in cs:
            if c == 7 or (r, c) == (9, 4):      # column 7 stays empty, (9, 4) is the stored zero added below
                continue
            rows.append(r); cols.append(int(c)); vals.append(float(rng.standard_normal()))
    rows += [2, 2, 2]; cols += [11, 11, 11]; vals += [0.5, 0.25, 2.0]
    rows += [9]; cols += [4]; vals += [0.0]
    perm = rng.permutation(len(rows))
    return (np.array(rows)[perm], np.array(cols)[perm], np.array(vals, dtype=np.float32)[perm])


def _dense(rows, cols, vals):
    d = np.zeros((N, F), dtype=np.float64)
    np.add.at(d, (rows, cols), vals.astype(np.float64))
    return d


def _csr_arrays(rows, cols, vals):
    """CSR arrays with the entries of a row in the (scrambled) order given: unsorted columns, duplicates kept."""
    order = np.argsort(rows, kind="stable")
    rowptr = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=N), out=rowptr[1:])
    return rowptr, cols[order], vals[order]


def _same(a: SparseFeatures, b: SparseFeatures):
    assert a.shape == b.shape and a.nnz == b.nnz
    assert torch.equal(a.rowptr, b.rowptr) and torch.equal(a.colidx, b.colidx)
    np.testing.assert_allclose(a.values.numpy(), b.values.numpy(), rtol=1e-6, atol=0)


def test_constructors_agree_and_canonicalise():
    rows, cols, vals = _entries()
    want = _dense(rows, cols, vals)
    rowptr, ci, cv = _csr_arrays(rows, cols, vals)
    a = SparseFeatures.from_arrays(rowptr, ci, cv, F)
    assert a.shape == (N, F) and a.device.type == "cpu" and not a.is_cuda
    assert a.rowptr.dtype == torch.int64 and a.colidx.dtype == torch.int32 and a.values.dtype == torch.float32
    np.testing.assert_allclose(a.to_dense().numpy(), want, rtol=1e-6, atol=1e-7)
    deg = (a.rowptr[1:] - a.rowptr[:-1]).numpy()
    assert deg[3] == 0 and deg[5] == F - 1                      # the empty and the full row
    assert not bool((a.colidx == 7).any())                      # the empty column
    for r in range(N):                                          # ascending columns, no repeated entry
        c = a.colidx[a.rowptr[r]:a.rowptr[r + 1]].numpy()
        assert (np.diff(c) > 0).all(), r
    at = int(a.rowptr[2]) + int(np.searchsorted(a.colidx[a.rowptr[2]:a.rowptr[3]].numpy(), 11))
    assert int(a.colidx[at]) == 11 and abs(float(a.values[at]) - want[2, 11]) < 1e-6      # the duplicates, summed
    at = int(a.rowptr[9]) + int(np.searchsorted(a.colidx[a.rowptr[9]:a.rowptr[10]].numpy(), 4))
    assert int(a.colidx[at]) == 4 and float(a.values[at]) == 0.0                          # the stored zero is kept
    assert a.nnz == np.count_nonzero(want) + 1

    coo = torch.sparse_coo_tensor(np.stack([rows, cols]), vals, (N, F))                  # uncoalesced, duplicates
    _same(SparseFeatures.from_torch_sparse(coo), a)
    _same(SparseFeatures.from_torch_sparse(coo.coalesce()), a)
    coo3 = torch.sparse_coo_tensor(np.stack([np.zeros_like(rows), rows, cols]), vals, (1, N, F))
    _same(SparseFeatures.from_torch_sparse(coo3), a)
    csr = torch.sparse_csr_tensor(a.rowptr, a.colidx.long(), a.values, (N, F))
    _same(SparseFeatures.from_torch_sparse(csr), a)
    _same(SparseFeatures.from_scipy(sp.coo_matrix((vals, (rows, cols)), shape=(N, F))), a)
    _same(SparseFeatures.from_scipy(sp.csc_matrix(sp.coo_matrix((vals, (rows, cols)), shape=(N, F)))), a)
    d = SparseFeatures.from_dense(torch.tensor(want, dtype=torch.float32))               # drops the stored zero
    assert d.nnz == a.nnz - 1
    np.testing.assert_allclose(d.to_dense().numpy(), want, rtol=1e-6, atol=1e-7)
    assert torch.equal(SparseFeatures.from_dense(torch.tensor(want, dtype=torch.float32)[None]).colidx, d.colidx)
    with pytest.raises(ValueError, match="batch size"):
        SparseFeatures.from_torch_sparse(torch.sparse_coo_tensor(np.zeros((3, 1), dtype=np.int64), [1.0], (2, N, F)))


def test_values_none_is_all_ones():
    rows, cols, vals = _entries()
    rowptr, ci, _ = _csr_arrays(rows, cols, vals)
    uniq = SparseFeatures.from_arrays(rowptr, ci, np.ones_like(vals), F)      # with the duplicates: (2, 11) counts 3
    binary = SparseFeatures.from_arrays(uniq.rowptr, uniq.colidx, None, F)
    assert binary.values is None and binary.nnz == uniq.nnz
    ones = SparseFeatures.from_arrays(uniq.rowptr, uniq.colidx, torch.ones(uniq.nnz), F)
    assert torch.equal(binary.to_dense(), ones.to_dense())
    assert float(binary.to_dense().sum()) == binary.nnz
    assert float(uniq.to_dense()[2, 11]) == 3.0
    summed = SparseFeatures.from_arrays(rowptr, ci, None, F)                  # repeated binary entries are summed too
    assert torch.equal(summed.to_dense(), uniq.to_dense())
    assert binary.transposed()["values_t"] is None
    sl = binary.rows(4, 20)
    assert sl.shape == (16, F) and torch.equal(sl.to_dense(), binary.to_dense()[4:20])
    assert sl.colidx.data_ptr() == binary.colidx[int(binary.rowptr[4]):].data_ptr()      # a view
    with pytest.raises(ValueError, match="rows"):
        binary.rows(5, N + 1)


def test_transposed_and_chunk_table(monkeypatch):
    rows, cols, vals = _entries()
    a = SparseFeatures.from_arrays(*_csr_arrays(rows, cols, vals), F)
    monkeypatch.setattr(ops, "SPARSE_COL_CHUNK", 4)
    t = a.transposed()
    assert t is a.transposed()                                            # cached
    assert t["col_chunk"] == 4
    colptr, rowidx = t["colptr"].numpy(), t["rowidx"].numpy()
    assert t["colptr"].dtype == torch.int64 and t["rowidx"].dtype == torch.int32
    assert colptr.shape == (F + 1,) and colptr[0] == 0 and colptr[-1] == a.nnz
    dt = np.zeros((F, N))
    for f in range(F):
        r = rowidx[colptr[f]:colptr[f + 1]]
        assert (np.diff(r) > 0).all(), f                                 # ascending rows within a column
        dt[f, r] = t["values_t"].numpy()[colptr[f]:colptr[f + 1]]
    np.testing.assert_array_equal(dt, a.to_dense().numpy().T)
    lens = np.diff(colptr)
    long_cols = np.nonzero(lens > 4)[0]
    assert len(long_cols) > 3 and t["n_long"] == len(long_cols)
    np.testing.assert_array_equal(t["long_cols"].numpy(), long_cols)
    assert t["long_cols"].dtype == torch.int32 and t["chunk_col"].dtype == torch.int32
    lp, cc = t["long_ptr"].numpy(), t["chunk_col"].numpy()
    cs, ce = t["chunk_start"].numpy(), t["chunk_end"].numpy()
    assert lp[0] == 0 and lp[-1] == t["n_chunks"] == len(cc) == len(cs) == len(ce)
    for i, f in enumerate(long_cols):                                     # every entry exactly once, in order
        at = colptr[f]
        assert lp[i + 1] - lp[i] == -(-lens[f] // 4)
        for c in range(lp[i], lp[i + 1]):
            assert cc[c] == f and cs[c] == at and 0 < ce[c] - cs[c] <= 4
            at = ce[c]
        assert at == colptr[f + 1]
    monkeypatch.setattr(ops, "SPARSE_COL_CHUNK", 10 ** 6)
    t2 = a.transposed()
    assert t2["n_long"] == 0 and t2["n_chunks"] == 0 and t2["chunk_col"] is None
    assert torch.equal(t2["rowidx"], t["rowidx"])


def test_validation_errors():
    rp, ci, v = [0, 2, 3], [0, 4, 1], [1.0, 2.0, 3.0]
    assert SparseFeatures.from_arrays(rp, ci, v, 5).nnz == 3
    with pytest.raises(ValueError, match=r"rowptr\[0\] must be 0.*got 1"):
        SparseFeatures.from_arrays([1, 2, 3], ci, v, 5)
    with pytest.raises(ValueError, match="rowptr.*nnz.*2"):
        SparseFeatures.from_arrays([0, 1, 2], ci, v, 5)
    with pytest.raises(ValueError, match=r"non-decreasing: rowptr\[2\] = 1 < rowptr\[1\] = 2"):
        SparseFeatures.from_arrays([0, 2, 1, 3], ci, v, 5)
    with pytest.raises(ValueError, match=r"column index out of range \[0,4\): \[0,4\]"):
        SparseFeatures.from_arrays(rp, ci, v, 4)
    with pytest.raises(ValueError, match=r"column index out of range \[0,5\): \[-1,4\]"):
        SparseFeatures.from_arrays(rp, [0, 4, -1], v, 5)
    with pytest.raises(ValueError, match="2147483648"):
        SparseFeatures.from_arrays(rp, ci, v, 1 << 31)
    with pytest.raises(ValueError, match="2147483648"):
        SparseFeatures._from_coo(torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), None, 1 << 31, 5)
    with pytest.raises(ValueError, match="finite: entry 1 is (inf|nan)"):
        SparseFeatures.from_arrays(rp, ci, [1.0, float("inf"), 3.0], 5)
    with pytest.raises(ValueError, match="finite: entry 2 is nan"):
        SparseFeatures.from_arrays(rp, ci, [1.0, 2.0, float("nan")], 5)
    with pytest.raises(ValueError, match=r"values: shape \(2,\), expected \(3,\)"):
        SparseFeatures.from_arrays(rp, ci, [1.0, 2.0], 5)
    with pytest.raises(ValueError, match="layout"):
        SparseFeatures.from_torch_sparse(torch.zeros(3, 4))


def test_bag_of_words_reproducible_and_sliceable():
    n, f = synth.ROW_BLOCK + 1000, 300
    a = synth.bag_of_words(n, f, 6, seed=3)
    b = synth.bag_of_words(n, f, 6, seed=3)
    assert a.values is None and a.shape == (n, f)
    assert torch.equal(a.rowptr, b.rowptr) and torch.equal(a.colidx, b.colidx)
    assert not torch.equal(a.colidx[:1000], synth.bag_of_words(n, f, 6, seed=4).colidx[:1000])
    deg = a.rowptr[1:] - a.rowptr[:-1]
    assert int(deg.max()) <= 6 and int(deg.min()) >= 1
    lens = torch.bincount(a.colidx.long(), minlength=f)
    assert int(lens[0]) > 20 * int(lens[f // 2:].max())                # Zipf columns: a few are long
    r0, r1 = synth.ROW_BLOCK - 700, synth.ROW_BLOCK + 300               # across a block boundary
    part, ref = synth.bag_of_words(n, f, 6, seed=3, rows=(r0, r1)), a.rows(r0, r1)
    assert part.shape == (r1 - r0, f)
    assert torch.equal(part.rowptr, ref.rowptr) and torch.equal(part.colidx, ref.colidx)
    c = synth.bag_of_words(2000, f, 6, seed=3, binary=False)
    assert c.values is not None and float(c.values.sum()) == 2000 * 6   # counts: every draw is in
    assert torch.equal(c.colidx, synth.bag_of_words(2000, f, 6, seed=3).colidx)


def test_partition_guard_raises_without_a_gpu():
    from han_amd.gat import HeteGAT_multi
    from han_amd.trainer import HANTrainer
    x = synth.bag_of_words(40, 12, 3, seed=1)
    dense = x.to_dense()
    model = HeteGAT_multi().build(2, 12, 3, (8,), (8, 1), 16, device="cpu")
    part = types.SimpleNamespace(active=True)      # stands for a dist.NodePartition of more than one rank
    labels, mask = torch.zeros(40, dtype=torch.int32), torch.ones(40, dtype=torch.uint8)
    msg = "sparse features under a node partition"
    with pytest.raises(NotImplementedError, match=msg):
        HANTrainer(model, [x, x], [None, None], labels, mask, part=part)
    with pytest.raises(NotImplementedError, match=msg):
        HANTrainer(model, [dense, x.to_dense().to_sparse()], [None, None], labels, mask, part=part)
    with pytest.raises(NotImplementedError, match=msg):
        HANTrainer(model, None, [None, None], labels, mask, part=part, xs_full=[x, x])
    assert model.partition is None                  # raised before the trainer touched the model's partition
    model.partition = part
    with pytest.raises(NotImplementedError, match=msg):
        model.node_level([dense, x], [None, None], 0.0, 0.0, False, ops.ACT_ELU)
    model.partition = None
    with pytest.raises(NotImplementedError, match=msg):
        model.node_level([dense, dense], [None, None], 0.0, 0.0, False, ops.ACT_ELU, xs_full=[x, x])


@pytest.mark.skipif(torch.cuda.is_available(), reason="dummy pointers: only where no launch can start")
def test_sparse_entry_points_validate_before_any_launch():
    """Return codes of han_project_sparse_fwd / _bwd; every call returns while the library validates (the pointers
    are dummy values, never dereferenced)."""
    from han_amd import _lib
    _lib.build()
    lib = _lib.load()
    P = 0x10000
    fwd = dict(rowptr=P, colidx=P, vals=None, W=P, a1=P, a2=P, b1=P, b2=P, H=P, table_dtype=0, f1=P, f2=P, N=100, F=37,
               K=8, FP=8, in_drop=0.0, fts_drop=0.0, seed=0, seed_dev=None, row_offset=0, flags=0, stream=None)
    bwd = dict(colptr=P, rowidx=P, vals_t=None, col_chunk=512, n_long=1, n_chunks=3, long_cols=P, long_ptr=P, chunk_col=P,
               chunk_start=P, chunk_end=P, dH=P, dW=P, workspace=None, workspace_bytes=0, N=100, F=37, K=8, FP=8,
               in_drop=0.0, seed=0, seed_dev=None, row_offset=0, stream=None)
    call = lambda name, base, **over: getattr(lib, name)(*{**base, **over}.values())
    assert call("han_project_sparse_fwd", fwd, N=0, rowptr=None, K=8, FP=4, in_drop=1.0) == 0      # N == 0: at once
    for over, code in ((dict(rowptr=None), -1), (dict(W=None), -1), (dict(f2=None), -1), (dict(N=-1), -1),
                       (dict(F=0), -1), (dict(N=1 << 31), -2), (dict(K=8, FP=4), -2), (dict(table_dtype=7), -2),
                       (dict(in_drop=1.0), -1), (dict(fts_drop=-0.1), -1), (dict(W=None, K=8, FP=4), -1)):
        assert call("han_project_sparse_fwd", fwd, **over) == code, over
    assert lib.han_project_sparse_bwd_workspace(0) == 0 and lib.han_project_sparse_bwd_workspace(3) == 3 * 64 * 4
    for over, code in ((dict(), -3), (dict(workspace=P, workspace_bytes=3 * 256 - 1), -3), (dict(colptr=None), -1),
                       (dict(dW=None), -1), (dict(dH=None), -1), (dict(col_chunk=0), -1), (dict(n_chunks=0), -1),
                       (dict(chunk_col=None), -1), (dict(long_ptr=None), -1), (dict(N=1 << 31), -2),
                       (dict(K=3, FP=21), -2), (dict(in_drop=1.0), -1), (dict(F=0), -1)):
        assert call("han_project_sparse_bwd", bwd, **over) == code, over
