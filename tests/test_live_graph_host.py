"""CSRGraph.with_live_columns against a numpy restatement: the entries whose column is live, in their order, with their
values; rows that lose every entry stay as empty rows; column ids and n_cols unchanged."""
import numpy as np
import pytest
import torch

from han_amd.graph import CSRGraph


def _ragged(seed, n_rows=37, n_cols=29, valued=False):
    """Rows of 0 .. 9 entries in no particular column order, with repeated columns, two of them empty."""
    rng = np.random.default_rng(seed)
    deg = rng.integers(0, 10, n_rows)
    deg[[3, n_rows - 1]] = 0
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    colidx = rng.integers(0, n_cols, int(deg.sum())).astype(np.int32)
    vals = rng.standard_normal(colidx.size).astype(np.float32) if valued else None
    g = CSRGraph(torch.from_numpy(rowptr), torch.from_numpy(colidx), n_cols,
                 values=torch.from_numpy(vals) if valued else None)
    return g, rowptr, colidx, vals


def _restate(rowptr, colidx, vals, live):
    rp, ci, va = [0], [], []
    for i in range(len(rowptr) - 1):
        for e in range(rowptr[i], rowptr[i + 1]):
            if live[colidx[e]]:
                ci.append(colidx[e])
                if vals is not None:
                    va.append(vals[e])
        rp.append(len(ci))
    return np.array(rp, np.int64), np.array(ci, np.int32), (np.array(va, np.float32) if vals is not None else None)


@pytest.mark.parametrize("valued", [False, True])
@pytest.mark.parametrize("frac", [0.1, 0.5])
def test_live_columns_equal_the_restatement(valued, frac):
    g, rowptr, colidx, vals = _ragged(7, valued=valued)
    live = np.random.default_rng(11).random(g.n_cols) < frac
    out = g.with_live_columns(torch.from_numpy(live.astype(np.uint8)))
    rp, ci, va = _restate(rowptr, colidx, vals, live)
    assert out.n_rows == g.n_rows and out.n_cols == g.n_cols and out.nnz == ci.size and not out.masked
    assert out.rowptr.dtype == torch.int64 and out.colidx.dtype == torch.int32
    assert np.array_equal(out.rowptr.numpy(), rp) and np.array_equal(out.colidx.numpy(), ci)
    assert (out.values is None) if not valued else np.array_equal(out.values.numpy(), va)
    assert (np.diff(rp) == 0).sum() > 2          # rows that lost every entry are still rows
    out.validate()
    # an ordinary graph: the bins and the chunks of its own rows, cached
    bins = out.row_bins(4, 6)
    assert bins is out.row_bins(4, 6)
    deg = np.diff(rp)
    # (its empty rows go with the wave-a-row bin: the four-rows-a-wave launch would read table row 0 for them)
    assert bins["n_short"] == int(((deg < 4) & (deg > 0)).sum())
    assert bins["n_mid"] == int((((deg >= 4) & (deg <= 6)) | (deg == 0)).sum())
    assert not np.isin(np.nonzero(deg == 0)[0], bins["short_rows"].numpy()).any()
    assert np.isin(np.nonzero(deg == 0)[0], bins["mid_rows"].numpy()).all()
    sp = out.row_split(6, 4)
    assert (sp is None) == (not (deg > 6).any())
    if sp is not None:
        assert np.array_equal(sp["long_rows"].numpy(), np.nonzero(deg > 6)[0])


def test_a_bool_mask_and_the_uint8_mask_agree():
    g, *_ = _ragged(3)
    live = np.random.default_rng(5).random(g.n_cols) < 0.3
    a = g.with_live_columns(torch.from_numpy(live))
    b = g.with_live_columns(torch.from_numpy(live.astype(np.uint8)))
    assert torch.equal(a.rowptr, b.rowptr) and torch.equal(a.colidx, b.colidx)


@pytest.mark.parametrize("valued", [False, True])
def test_all_live_gives_an_equal_graph(valued):
    g, *_ = _ragged(9, valued=valued)
    out = g.with_live_columns(torch.ones(g.n_cols, dtype=torch.uint8))
    assert torch.equal(out.rowptr, g.rowptr) and torch.equal(out.colidx, g.colidx) and out.n_cols == g.n_cols
    assert (out.values is None) if not valued else torch.equal(out.values, g.values)


@pytest.mark.parametrize("valued", [False, True])
def test_none_live_gives_an_empty_graph(valued):
    g, *_ = _ragged(13, valued=valued)
    out = g.with_live_columns(torch.zeros(g.n_cols, dtype=torch.uint8))
    assert out.nnz == 0 and out.n_rows == g.n_rows and out.n_cols == g.n_cols
    assert bool((out.rowptr == 0).all()) and out.colidx.numel() == 0
    assert (out.values is None) if not valued else out.values.numel() == 0
    out.validate()


def test_a_mask_of_another_length_is_an_error():
    g, *_ = _ragged(1)
    with pytest.raises(ValueError, match="live_mask"):
        g.with_live_columns(torch.ones(g.n_cols + 1, dtype=torch.uint8))


def test_the_transposed_live_graph_keeps_the_order_of_the_transposed_graph():
    """What the trainer builds: the transposed graph, filtered by live destination -- per source the live destinations in
    ascending order, i.e. the transposed image of the graph with only its live rows."""
    g, rowptr, colidx, _ = _ragged(21, n_rows=29, n_cols=29)
    live = np.random.default_rng(2).random(29) < 0.4
    lt = g.transpose().with_live_columns(torch.from_numpy(live))
    for j in range(29):
        want = sorted(i for i in range(29) if live[i] for e in range(rowptr[i], rowptr[i + 1]) if colidx[e] == j)
        assert lt.colidx[int(lt.rowptr[j]):int(lt.rowptr[j + 1])].tolist() == want, j
