"""CSRGraph.row_subset -- the degree bins and the long-row chunks restricted to a row list (HAN_FLAG_K2_ROW_SUBSET) --
against a brute-force partition of the listed rows by length.  Host tensors only."""
import numpy as np
import pytest
import torch

from tests import live_forward_cases as lc


def _graph():
    from han_amd.graph import CSRGraph
    rowptr, colidx, _ = lc.k2_graph("cpu")
    return CSRGraph(rowptr, colidx, lc.K2_N)


@pytest.mark.parametrize("which", lc.SUBSETS)
def test_restricted_bins_and_split_partition_the_listed_rows(which):
    g = _graph()
    deg = lc.k2_degrees()
    mask = lc.k2_subset(which)
    r = g.row_subset(torch.from_numpy(mask), 16, lc.SPLIT_DEG, lc.SPLIT_CHUNK)
    short, mid, long = lc.brute_force_sets(deg, mask, 16, lc.SPLIT_DEG)
    b = r["bins"]
    assert b["short_rows"].dtype == torch.int32 and b["mid_rows"].dtype == torch.int32      # never the identity form
    assert b["short_rows"].tolist() == short and b["n_short"] == len(short)
    assert b["mid_rows"].tolist() == mid and b["n_mid"] == len(mid)
    assert r["n_rows"] == int(mask.sum()) and r["nnz"] == int(deg[mask].sum())
    assert len(short) + len(mid) + len(long) == int(mask.sum())
    sp = r["split"]
    if not long:
        assert sp is None
        return
    assert sp["long_rows"].tolist() == long and sp["n_long"] == len(long) and sp["split_deg"] == lc.SPLIT_DEG
    rowptr = g.rowptr.numpy()
    starts, ends, owner = sp["chunk_start"].tolist(), sp["chunk_end"].tolist(), sp["chunk_long"].tolist()
    lp = sp["long_ptr"].tolist()
    assert lp[0] == 0 and lp[-1] == sp["n_chunks"] == len(starts)
    for k, row in enumerate(long):      # a row's chunks cover its entries in order, SPLIT_CHUNK at a time
        cs = list(range(lp[k], lp[k + 1]))
        assert len(cs) == -(-int(deg[row]) // lc.SPLIT_CHUNK) and all(owner[c] == k for c in cs)
        assert starts[cs[0]] == rowptr[row] and ends[cs[-1]] == rowptr[row + 1]
        assert all(ends[c] == starts[c + 1] for c in cs[:-1]) and all(0 < ends[c] - starts[c] <= lc.SPLIT_CHUNK for c in cs)


def test_the_full_list_gives_the_sets_of_the_whole_graph():
    """Every row listed: the restricted sets are the graph's own row_bins / row_split."""
    g = _graph()
    r = g.row_subset(torch.ones(lc.K2_N, dtype=torch.bool), 16, lc.SPLIT_DEG, lc.SPLIT_CHUNK)
    full_b, full_s = g.row_bins(16, lc.SPLIT_DEG), g.row_split(lc.SPLIT_DEG, lc.SPLIT_CHUNK)
    assert torch.equal(r["bins"]["short_rows"], full_b["short_rows"]) and torch.equal(r["bins"]["mid_rows"], full_b["mid_rows"])
    for k in ("long_rows", "long_ptr", "chunk_long", "chunk_start", "chunk_end"):
        assert torch.equal(r["split"][k], full_s[k]), k
    assert r["nnz"] == g.nnz


def test_a_mask_of_another_shape_is_refused():
    g = _graph()
    with pytest.raises(ValueError, match="rows"):
        g.row_subset(torch.ones(lc.K2_N + 1, dtype=torch.bool))
    with pytest.raises(ValueError, match="rows"):
        g.row_subset(torch.ones(lc.K2_N, dtype=torch.uint8))


def test_the_forward_bound_is_a_constant_of_its_own():
    from han_amd import trainer
    assert trainer.LIVE_FORWARD_MIN_ROWS == 262144
    assert "LIVE_FORWARD_MIN_ROWS" in vars(trainer) and trainer.LIVE_FORWARD_MIN_ROWS is not None


def test_bindings_and_flag_are_declared():
    import os
    from han_amd import _lib, ops
    assert "han_classifier_loss_live" in _lib.SIGNATURES
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "han_hip.h")).read()
    assert f"#define HAN_FLAG_K2_ROW_SUBSET {ops.FLAG_K2_ROW_SUBSET}" in hdr
    k2_flags = (ops.FLAG_XCD_ORDER, ops.FLAG_LEAN, ops.FLAG_K2_DEEP, ops.FLAG_K2_SHARED_HASH, ops.FLAG_MASKED_EDGES, 2048, 4096)
    assert all(ops.FLAG_K2_ROW_SUBSET & f == 0 for f in k2_flags)      # a free bit of the K2 flag word
