"""K0 meta-path construction, host side (no GPU): relation() on CPU tensors against NumPy, the meta-path plan (hops,
derived transposes, the palindromic H Hᵀ split, the left-to-right fallback), every ValueError of the builder, the
missing CPU path, and the synthetic heterogeneous workloads."""
import numpy as np
import pytest
import torch

from han_amd import metapath, ops, synth
from han_amd.graph import CSRGraph


def _ref_csr(src, dst, n_src):
    pairs = sorted(set(zip(np.asarray(src).tolist(), np.asarray(dst).tolist())))
    counts = np.bincount(np.array([s for s, _ in pairs], dtype=np.int64), minlength=n_src)
    rowptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return rowptr, np.array([d for _, d in pairs], dtype=np.int32)


def _rel(src, dst, n_src, n_dst):
    return metapath.relation(np.asarray(src), np.asarray(dst), n_src, n_dst)


@pytest.fixture()
def small():
    """4 authors, 6 papers, 2 conferences, 3 terms."""
    return {"AP": _rel([0, 0, 1, 2, 2, 3], [0, 1, 1, 2, 3, 5], 4, 6),
            "PC": _rel([0, 1, 2, 3, 4, 5], [0, 0, 1, 1, 0, 1], 6, 2),
            "PT": _rel([0, 1, 2, 5, 5], [0, 2, 2, 1, 0], 6, 3)}


def test_relation_sorts_and_drops_repeated_edges():
    rng = np.random.default_rng(0)
    src, dst = rng.integers(0, 37, 500), rng.integers(0, 11, 500)      # many repeats, no order
    rp, ci = _ref_csr(src, dst, 40)
    for s, d in ((src, dst), (torch.as_tensor(src), torch.as_tensor(dst, dtype=torch.int32)),
                 (src.astype(np.int32), dst.astype(np.int16))):
        g = metapath.relation(s, d, 40, 11)
        assert (g.n_rows, g.n_cols, g.values, g.device.type) == (40, 11, None, "cpu")
        assert g.rowptr.dtype == torch.int64 and g.colidx.dtype == torch.int32
        np.testing.assert_array_equal(g.rowptr.numpy(), rp)
        np.testing.assert_array_equal(g.colidx.numpy(), ci)


def test_relation_of_no_edges_and_isolated_nodes():
    g = metapath.relation(np.zeros(0, np.int64), np.zeros(0, np.int64), 5, 3)
    assert g.nnz == 0 and g.rowptr.tolist() == [0] * 6
    g = metapath.relation([4, 4, 0], [2, 0, 2], 6, 3)
    assert g.rowptr.tolist() == [0, 1, 1, 1, 1, 3, 3] and g.colidx.tolist() == [2, 0, 2]


@pytest.mark.parametrize("src,dst", [([0, 5], [0, 1]), ([-1, 0], [0, 0]), ([0, 1], [3, 0]), ([0, 1], [0, -2])])
def test_relation_rejects_ids_out_of_range(src, dst):
    with pytest.raises(ValueError, match="outside"):
        metapath.relation(np.array(src), np.array(dst), 5, 3)


def test_relation_rejects_malformed_edge_lists():
    with pytest.raises(ValueError, match="ids"):
        metapath.relation([0, 1], [0], 2, 2)
    with pytest.raises(ValueError, match="integer"):
        metapath.relation(np.array([0.0, 1.0]), np.array([0, 1]), 2, 2)
    with pytest.raises(ValueError, match="1-D"):
        metapath.relation(np.zeros((2, 2), np.int64), np.zeros((2, 2), np.int64), 2, 2)


def test_plan_splits_palindromes_at_the_middle(small):
    p = metapath.plan(small, "APA")
    assert p["hops"] == [("AP", False), ("AP", True)] and p["split"] == 1
    p = metapath.plan(small, "APCPA")
    assert p["hops"] == [("AP", False), ("PC", False), ("PC", True), ("AP", True)] and p["split"] == 2
    assert metapath.plan(small, "APTPA")["split"] == 2
    assert metapath.plan(small, "APTPA")["sizes"] == {"A": 4, "P": 6, "C": 2, "T": 3}
    # PAP over a given "PA" (the pap-3m form): P -> A direct, A -> P derived
    pa = {"PA": small["AP"].transpose()}
    p = metapath.plan(pa, "PAP")
    assert p["hops"] == [("PA", False), ("PA", True)] and p["split"] == 1


def test_plan_falls_back_left_to_right(small):
    # PAP over "AP": the SECOND half is the relation as given, the first half derived
    p = metapath.plan(small, "PAP")
    assert p["hops"] == [("AP", True), ("AP", False)] and p["split"] is None
    assert metapath.plan(small, "APC")["split"] is None                      # not a palindrome
    assert metapath.plan(small, "APCP")["split"] is None
    assert metapath.plan(small, "CPAPC")["split"] is None                    # palindrome, second half direct
    rel = dict(small, PP=_rel([0, 1], [1, 0], 6, 6))
    p = metapath.plan(rel, "APPA")                                          # even length: the middle hop is real
    assert p["hops"] == [("AP", False), ("PP", False), ("AP", True)] and p["split"] is None


def test_plan_errors(small):
    with pytest.raises(ValueError, match="both directions"):
        metapath.plan(dict(small, PA=small["AP"].transpose()), "APA")
    with pytest.raises(ValueError, match="no relation between 'C' and 'T'"):
        metapath.plan(small, "APCT")
    with pytest.raises(ValueError, match="nodes"):
        metapath.plan(dict(small, PC=_rel([0], [0], 7, 2)), "APA")          # 6 papers in AP, 7 in PC
    with pytest.raises(ValueError, match="nodes"):
        metapath.plan({"AP": small["AP"], "TA": _rel([0], [0], 3, 5)}, "APA")   # 4 authors in AP, 5 in TA
    with pytest.raises(ValueError, match="ordered pair"):
        metapath.plan({"APC": small["AP"]}, "APA")
    with pytest.raises(ValueError, match="CSRGraph"):
        metapath.plan({"AP": (small["AP"].rowptr, small["AP"].colidx)}, "APA")
    with pytest.raises(ValueError, match="at least two"):
        metapath.plan(small, "A")
    # the same errors come from metapath_graph, before anything else
    with pytest.raises(ValueError, match="both directions"):
        metapath.metapath_graph(dict(small, PA=small["AP"].transpose()), "APA")
    with pytest.raises(ValueError, match="no relation"):
        metapath.metapath_graph(small, "APX")
    with pytest.raises(ValueError, match="ends on the type"):
        metapath.metapath_graph(small, "APC")


def test_compose_checks_the_chain(small):
    with pytest.raises(ValueError, match="columns"):
        metapath.compose([small["AP"], small["AP"]])
    with pytest.raises(ValueError, match="square"):
        metapath.compose([small["AP"], small["PC"]], self_loops=True)
    with pytest.raises(ValueError, match="no graphs"):
        metapath.compose([])


def test_no_cpu_path(small):
    with pytest.raises(ValueError, match="no CPU path"):
        metapath.compose([small["AP"], small["PC"]])
    with pytest.raises(ValueError, match="no CPU path"):
        metapath.compose([small["AP"]])
    with pytest.raises(ValueError, match="no CPU path"):
        metapath.metapath_graph(small, "APA")
    with pytest.raises(ValueError, match="no CPU path"):
        metapath.metapath_graph(small, "APC", self_loops=False)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.csr_bool_matmul(small["AP"], small["PC"])


def test_binning_constants_fit_the_abi():
    assert 0 <= ops.SPGEMM_SHORT <= ops.SPGEMM_MAX_SHORT
    assert 32 <= ops.SPGEMM_TILE <= ops.SPGEMM_MAX_TILE and ops.SPGEMM_TILE % 32 == 0
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "han_hip.h")).read()
    assert int(re.search(r"#define HAN_SPGEMM_DIAG (\d+)", hdr).group(1)) == ops.SPGEMM_DIAG
    assert int(re.search(r"#define HAN_SPGEMM_MAX_SHORT (\d+)", hdr).group(1)) == ops.SPGEMM_MAX_SHORT
    assert 1 << int(re.search(r"#define HAN_SPGEMM_MAX_TILE \(1 << (\d+)\)", hdr).group(1)) == ops.SPGEMM_MAX_TILE


def test_hetero_relations_dblp_like():
    rel, sizes = synth.hetero_relations("dblp-like")
    assert sizes == {"A": 4057, "P": 14328, "C": 20, "T": 8000}
    assert sorted(rel) == ["AP", "PC", "PT"]
    for key, g in rel.items():
        assert (g.n_rows, g.n_cols) == (sizes[key[0]], sizes[key[1]])
        g.validate()
        c, rows = g.colidx.long(), torch.repeat_interleave(torch.arange(g.n_rows), g.degrees())
        assert bool(((c[1:] > c[:-1]) | (rows[1:] != rows[:-1])).all())   # strictly increasing inside every row
    assert int(rel["AP"].degrees().min()) >= 1                              # every author writes
    assert bool((rel["PC"].degrees() == 1).all())                           # one conference per paper
    again, _ = synth.hetero_relations("dblp-like")
    other, _ = synth.hetero_relations("dblp-like", seed=1)
    assert all(torch.equal(rel[k].colidx, again[k].colidx) for k in rel)
    assert not torch.equal(rel["PT"].colidx, other["PT"].colidx) or not torch.equal(rel["PT"].rowptr, other["PT"].rowptr)
    with pytest.raises(ValueError, match="unknown"):
        synth.hetero_relations("dblp")
