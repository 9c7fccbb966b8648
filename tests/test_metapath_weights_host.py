"""Weighted meta-path graphs (K0), host side (no GPU): every ValueError of the new arguments and ops, plan()
untouched by them, and the NumPy references of tests/metapath_weights_ref.py -- which the GPU tests compare the
kernels with -- against brute-force dense computations on the 4-author fixture of tests/test_metapath_host.py."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from han_amd import metapath, ops
from han_amd.graph import CSRGraph
from tests import metapath_weights_ref as ref


def _rel(src, dst, n_src, n_dst):
    return metapath.relation(np.asarray(src), np.asarray(dst), n_src, n_dst)


@pytest.fixture()
def small():
    """4 authors, 6 papers, 2 conferences, 3 terms."""
    return {"AP": _rel([0, 0, 1, 2, 2, 3], [0, 1, 1, 2, 3, 5], 4, 6),
            "PC": _rel([0, 1, 2, 3, 4, 5], [0, 0, 1, 1, 0, 1], 6, 2),
            "PT": _rel([0, 1, 2, 5, 5], [0, 2, 2, 1, 0], 6, 3)}


def _dense(g: CSRGraph):
    d = np.zeros((g.n_rows, g.n_cols), dtype=np.int64)
    rows = np.repeat(np.arange(g.n_rows), g.degrees().numpy())
    np.add.at(d, (rows, g.colidx.numpy()), 1)
    return d


def test_weights_and_top_k_arguments_are_checked(small):
    for call in (lambda **kw: metapath.metapath_graph(small, "APA", **kw),
                 lambda **kw: metapath.compose([small["AP"], small["AP"].transpose()], **kw)):
        with pytest.raises(ValueError, match="weights"):
            call(weights="counts")
        with pytest.raises(ValueError, match="weights"):
            call(weights=True)
    with pytest.raises(ValueError, match="backwards"):
        metapath.metapath_graph(small, "APC", self_loops=False, weights="pathsim")
    with pytest.raises(ValueError, match="square"):
        metapath.compose([small["AP"], small["PC"]], weights="pathsim")
    with pytest.raises(ValueError, match="top_k needs weights"):
        metapath.metapath_graph(small, "APA", top_k=4)
    for k in (0, -3, 1.5):
        with pytest.raises(ValueError, match="top_k"):
            metapath.metapath_graph(small, "APA", weights="count", top_k=k)
    # the checks of the boolean builder still come first / still hold
    with pytest.raises(ValueError, match="no relation"):
        metapath.metapath_graph(small, "APX", weights="count")
    with pytest.raises(ValueError, match="ends on the type"):
        metapath.metapath_graph(small, "APC", weights="count")


@pytest.mark.parametrize("weights", ["count", "pathsim"])
def test_no_cpu_path(small, weights):
    with pytest.raises(ValueError, match="no CPU path"):
        metapath.metapath_graph(small, "APCPA", weights=weights, top_k=2)
    with pytest.raises(ValueError, match="no CPU path"):
        metapath.compose([small["AP"], small["AP"].transpose()], weights=weights)
    with pytest.raises(ValueError, match="no CPU path"):
        metapath.compose([small["AP"]], weights="count")


def test_new_ops_reject_cpu_graphs_and_bad_arguments(small):
    ap = small["AP"]
    with pytest.raises(ValueError, match="no CPU path"):
        ops.csr_count_matmul(ap, ap.transpose())
    with pytest.raises(ValueError, match="CSRGraph"):
        ops.csr_count_matmul((ap.rowptr, ap.colidx), ap)
    sq = CSRGraph(torch.tensor([0, 2, 3]), torch.tensor([0, 1, 1], dtype=torch.int32), 2,
                  values=torch.tensor([1.0, 2.0, 3.0]))
    with pytest.raises(ValueError, match="no CPU path"):
        ops.csr_pathsim(sq, torch.tensor([1, 2, 3]))
    with pytest.raises(ValueError, match="no CPU path"):
        ops.csr_row_topk(sq, 1)
    for k in (0, -1, 2.5):
        with pytest.raises(ValueError, match="k ="):
            ops.csr_row_topk(sq, k)
    with pytest.raises(ValueError, match="no values"):
        ops.csr_row_topk(CSRGraph(sq.rowptr, sq.colidx, 2), 1)
    with pytest.raises(ValueError, match="square"):
        ops.csr_pathsim(ap, torch.ones(ap.nnz, dtype=torch.int64))


def test_plan_is_untouched_by_the_new_arguments(small):
    import inspect
    assert list(inspect.signature(metapath.plan).parameters) == ["relations", "metapath"]
    assert metapath.plan(small, "APCPA") == dict(hops=[("AP", False), ("PC", False), ("PC", True), ("AP", True)],
                                                 split=2, sizes={"A": 4, "P": 6, "C": 2, "T": 3})
    assert metapath.plan(small, "PAP")["split"] is None
    assert metapath.WEIGHTS == (None, "count", "pathsim")
    assert ops.SPGEMM_DIAG == 1 and (ops.SPGEMM_SHORT, ops.SPGEMM_TILE) == (1024, 1 << 17)


@pytest.mark.parametrize("mp", ["APA", "APCPA", "APTPA"])
def test_references_agree_with_dense_brute_force(small, mp):
    n = 4
    hops = [small[k].transpose() if t else small[k] for k, t in metapath.plan(small, mp)["hops"]]
    dense = _dense(hops[0])
    for g in hops[1:]:
        dense = dense @ _dense(g)
    sps = [sp.csr_matrix((np.ones(g.nnz, dtype=np.int64), g.colidx.numpy(), g.rowptr.numpy()),
                         shape=(g.n_rows, g.n_cols)) for g in hops]
    for diag in (False, True):
        m = ref.count_chain(sps, diag=diag)
        present = (dense != 0) | (np.eye(n, dtype=bool) & diag)
        want = [(i, j, int(dense[i, j])) for i in range(n) for j in range(n) if present[i, j]]
        rows = np.repeat(np.arange(n), np.diff(m.indptr))
        assert list(zip(rows.tolist(), m.indices.tolist(), m.data.tolist())) == want
        assert m.data.dtype == np.int64
    # author 3 wrote paper 5 alone; authors 0 and 1 share paper 1
    assert dense[0, 1] >= 1 and dense[3, 3] >= 1
    # PathSim: the formula entry by entry in Python floats (doubles), rounded once
    w = ref.pathsim(m.indptr, m.indices, m.data)
    for e, (i, j, c) in enumerate(want):
        assert w[e] == (np.float32(1.0) if i == j else np.float32(2.0 * c / (int(dense[i, i]) + int(dense[j, j]))))
    assert w.dtype == np.float32
    # top-k: sorted() by (-value, column) over the entries off the diagonal
    for k in (1, 2, 10):
        for keep_diag in (True, False):
            ptr, cols, vals = ref.topk(m.indptr, m.indices, w, k, keep_diag)
            for i in range(n):
                row = [(j, w[e]) for e, (r, j, _) in enumerate(want) if r == i]
                best = sorted((x for x in row if x[0] != i), key=lambda x: (-x[1], x[0]))[:k]
                kept = sorted(best + ([x for x in row if x[0] == i] if keep_diag else []))
                assert list(zip(cols[ptr[i]:ptr[i + 1]].tolist(), vals[ptr[i]:ptr[i + 1]].tolist())) == kept


def test_reference_edge_cases():
    # a row without instances: the added diagonal counts 0 and its PathSim is 1; ties go to the smaller column
    m = ref.counted(sp.csr_matrix(np.array([[2, 1, 1, 0], [1, 3, 0, 0], [1, 0, 1, 0], [0, 0, 0, 0]])), diag=True)
    assert m.indptr.tolist() == [0, 3, 5, 7, 8] and m.data.tolist() == [2, 1, 1, 1, 3, 1, 1, 0]
    w = ref.pathsim(m.indptr, m.indices, m.data)
    assert w[-1] == 1.0 and w[0] == 1.0 and w[1] == np.float32(2.0 / 5.0)
    keep = ref.topk_row([0, 1, 2, 3], np.float32([1.0, 0.5, 0.5, 0.5]), 0, 2)
    assert keep.tolist() == [0, 1, 2]
    assert ref.topk_row([0, 1, 2, 3], np.float32([1.0, 0.5, 0.7, 0.5]), 0, 1, keep_diag=False).tolist() == [2]
    assert ref.topk_row([1, 2], np.float32([0.1, 0.2]), 0, 5).tolist() == [0, 1]
