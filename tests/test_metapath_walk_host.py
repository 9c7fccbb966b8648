"""Sampled meta-path neighbours (K0), host side (no GPU): the NumPy restatement of tests/metapath_walk_ref.py -- which
the GPU tests compare the kernels with bit for bit -- against scipy products, against itself over row ranges, on the
fanout ties, and against the exact random-walk transition probabilities; and every ValueError of
metapath.metapath_sample / ops.metapath_walk, all raised before a GPU is asked for."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from han_amd import metapath, ops
from han_amd.graph import CSRGraph
from tests import metapath_walk_ref as ref


def _rows_to_csr(rows):
    rowptr = np.zeros(len(rows) + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum([len(r) for r in rows])
    colidx = np.concatenate([np.asarray(r, dtype=np.int32) for r in rows]) if rowptr[-1] else np.zeros(0, np.int32)
    return rowptr, colidx


def _transpose(rowptr, colidx, n_cols):
    rows = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    order = np.argsort(colidx, kind="stable")
    tp = np.zeros(n_cols + 1, dtype=np.int64)
    tp[1:] = np.cumsum(np.bincount(colidx, minlength=n_cols))
    return tp, rows[order].astype(np.int32)


def apcpa_chain(seed, n_a=60, n_p=90, n_c=5, max_ap=6, max_pc=2, empty=0.1):
    """The four hops AP, PC, PCᵀ, APᵀ of a random APCPA chain as (rowptr, colidx) pairs, and the sizes per hop: about
    `empty` of the authors / papers have no entry, the others 1 .. max entries drawn with repeats (parallel edges)."""
    rng = np.random.default_rng(seed)

    def rel(n_rows, n_cols, most):
        deg = np.where(rng.random(n_rows) < empty, 0, rng.integers(1, most + 1, n_rows))
        return _rows_to_csr([rng.integers(0, n_cols, d) for d in deg])

    ap, pc = rel(n_a, n_p, max_ap), rel(n_p, n_c, max_pc)
    return [ap, pc, _transpose(*pc, n_c), _transpose(*ap, n_p)], [n_a, n_p, n_c, n_p, n_a]


def _count_matrix(hop, n_cols):
    rowptr, colidx = hop
    m = sp.csr_matrix((np.ones(len(colidx), dtype=np.int64), colidx.copy(), rowptr.copy()),
                      shape=(len(rowptr) - 1, n_cols))
    m.sum_duplicates()             # (in place: on copies, the hops stay as stored)
    return m


def _rows_of(rowptr, colidx, visits):
    return [(colidx[s:e].tolist(), visits[s:e].tolist()) for s, e in zip(rowptr[:-1], rowptr[1:])]


def test_every_sampled_entry_is_an_entry_of_the_product():
    hops, sizes = apcpa_chain(5)
    prod = None
    for h, n in zip(hops, sizes[1:]):
        m = _count_matrix(h, n)
        prod = m if prod is None else prod @ m
    reach = (prod.toarray() != 0)
    for diag in (False, True):
        rowptr, colidx, visits = ref.sample(hops, 64, 5, seed=3, diag=diag)
        assert rowptr[0] == 0 and rowptr[-1] == len(colidx) == len(visits)
        assert colidx.dtype == np.int32 and visits.dtype == np.int32
        for i, (cols, cnt) in enumerate(_rows_of(rowptr, colidx, visits)):
            assert cols == sorted(set(cols))                                 # strictly ascending
            assert sum(cnt) <= 64 and len([c for c in cols if not (diag and c == i)]) <= 5
            for j, c in zip(cols, cnt):
                if diag and j == i:
                    assert c >= 0
                else:
                    assert reach[i, j] and c >= 1
            if diag:
                assert i in cols
        if not diag:
            assert any(len(c) == 0 for c, _ in _rows_of(rowptr, colidx, visits))    # an author without papers


def test_row_ranges_concatenate_to_the_whole_graph():
    hops, _ = apcpa_chain(6)
    for diag in (False, True):
        whole = ref.sample(hops, 100, 7, seed=11, diag=diag)
        a, b = ref.sample(hops, 100, 7, seed=11, diag=diag, rows=(0, 23)), \
            ref.sample(hops, 100, 7, seed=11, diag=diag, rows=(23, 60))
        np.testing.assert_array_equal(np.concatenate([a[0], a[0][-1] + b[0][1:]]), whole[0])
        np.testing.assert_array_equal(np.concatenate([a[1], b[1]]), whole[1])
        np.testing.assert_array_equal(np.concatenate([a[2], b[2]]), whole[2])
    other = ref.sample(hops, 100, 7, seed=12)
    assert not (len(other[1]) == len(whole[1]) and np.array_equal(other[2], whole[2]))


def test_fanout_keeps_the_right_ties():
    cols = [2, 3, 5, 7, 8, 9]
    cnt = [4, 1, 4, 9, 4, 1]
    assert ref.keep_row(cols, cnt, 0, 1, False).tolist() == [3]              # 7
    assert ref.keep_row(cols, cnt, 0, 2, False).tolist() == [0, 3]           # 7, then the first 4: column 2
    assert ref.keep_row(cols, cnt, 0, 3, False).tolist() == [0, 2, 3]
    assert ref.keep_row(cols, cnt, 0, 5, False).tolist() == [0, 1, 2, 3, 4]  # the 1 of column 3, not of 9
    assert ref.keep_row(cols, cnt, 0, 9, False).tolist() == [0, 1, 2, 3, 4, 5]
    # the diagonal stays whatever its count and takes no place
    assert ref.keep_row(cols, cnt, 3, 1, True).tolist() == [1, 3]
    assert ref.keep_row(cols, cnt, 7, 1, True).tolist() == [0, 3]
    assert ref.keep_row(cols, cnt, 7, 1, False).tolist() == [3]
    # one hop over a row with parallel edges: 3 of its 4 entries lead to column 1
    rowptr, colidx, visits = ref.sample([_rows_to_csr([[1, 0, 1, 1], []])], 4096, None, seed=0)
    assert rowptr.tolist() == [0, 2, 2] and colidx.tolist() == [0, 1] and visits.sum() == 4096
    assert abs(visits[1] / 4096 - 0.75) < 6 * np.sqrt(0.75 * 0.25 / 4096)
    # a square graph with the diagonal never visited: (i, i) joins with count 0, in column order
    rowptr, colidx, visits = ref.sample([_rows_to_csr([[1], [0, 2], []])], 8, 1, seed=0, diag=True)
    assert rowptr.tolist() == [0, 2, 4, 5] and colidx[:2].tolist() == [0, 1] and visits[:2].tolist() == [0, 8]
    assert colidx[4] == 2 and visits[4] == 0 and visits[2:4].sum() <= 8 and 1 in colidx[2:4]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_visit_frequencies_estimate_the_transition_probabilities(seed):
    """|c_ij / W - p_ij| <= 6 sqrt(p_ij (1 - p_ij) / W) for EVERY pair (the unreachable ones included: p = 0 allows no
    visit), p = the product of the row-normalised relations, W = 4096, every end point kept.  A condition, not a
    measurement: the inputs are fixed, and the normal tail at 6 sigma is 2e-9 per pair."""
    W = 4096
    hops, sizes = apcpa_chain(100 + seed)
    p = None
    for h, n in zip(hops, sizes[1:]):
        m = _count_matrix(h, n).toarray().astype(np.float64)
        deg = m.sum(1, keepdims=True)
        m = np.divide(m, deg, out=np.zeros_like(m), where=deg > 0)
        p = m if p is None else p @ m
    assert (np.diff(hops[0][0]) == 0).any() and (np.diff(hops[1][0]) == 0).any()     # dead ends at both levels
    rowptr, colidx, visits = ref.sample(hops, W, None, seed=seed)
    c = np.zeros_like(p)
    c[np.repeat(np.arange(sizes[0]), np.diff(rowptr)), colidx] = visits
    np.testing.assert_array_equal(c.sum(1) <= W, True)
    bound = 6.0 * np.sqrt(p * (1.0 - p) / W)
    dev = np.abs(c / W - p)
    worst = float((dev[bound > 0] / bound[bound > 0]).max())
    print(f"seed {seed}: {int((p > 0).sum())} reachable pairs, worst |c/W - p| / sigma = {6 * worst:.2f}")
    assert (dev <= bound).all()


# ---------------------------------------------------------------------------------------------- the argument checks
def _rel(src, dst, n_src, n_dst):
    return metapath.relation(np.asarray(src), np.asarray(dst), n_src, n_dst)


@pytest.fixture()
def small():
    """4 authors, 6 papers, 2 conferences (CPU graphs)."""
    return {"AP": _rel([0, 0, 1, 2, 2, 3], [0, 1, 1, 2, 3, 5], 4, 6),
            "PC": _rel([0, 1, 2, 3, 4, 5], [0, 0, 1, 1, 0, 1], 6, 2)}


def test_metapath_sample_checks_its_arguments_before_the_gpu(small):
    s = lambda mp="APCPA", **kw: metapath.metapath_sample(small, mp, **kw)
    for walks in (0, -1, 4097, 2.5, True):
        with pytest.raises(ValueError, match="walks"):
            s(walks=walks)
    for fanout in (0, -2, 257, 1.5, True):
        with pytest.raises(ValueError, match="fanout"):
            s(fanout=fanout)
    with pytest.raises(ValueError, match="fanout"):
        s(walks=8, fanout=9)
    for weights in ("pathsim", "counts", True, 1):
        with pytest.raises(ValueError, match="weights"):
            s(weights=weights)
    for seed in (-1, 1 << 64, 0.5):
        with pytest.raises(ValueError, match="seed"):
            s(seed=seed)
    with pytest.raises(ValueError, match="ends on the type"):
        s("APC")
    with pytest.raises(ValueError, match="no relation"):
        s("APX")
    with pytest.raises(ValueError, match="hops"):
        s("APAPAPAPAPA")                                                     # ten hops
    for rows in ((3, 2), (0, 5), (-1, 2), (0,), "ab", (0.5, 2), 3):
        with pytest.raises(ValueError, match="rows"):
            s(rows=rows)
    # every argument in order: only the device is wrong
    for kw in (dict(), dict(self_loops=False), dict(walks=4096, fanout=None, weights="prob", rows=(1, 3), seed=(1 << 64) - 1)):
        with pytest.raises(ValueError, match="no CPU path"):
            s(**kw)
    with pytest.raises(ValueError, match="no CPU path"):
        s("APC", self_loops=False, weights="count")
    assert metapath.SAMPLE_WEIGHTS == (None, "count", "prob") and metapath.WEIGHTS == (None, "count", "pathsim")


def test_ops_metapath_walk_checks_its_arguments_before_the_gpu(small):
    ap, pc = small["AP"], small["PC"]
    apt = ap.transpose()
    with pytest.raises(ValueError, match="hops"):
        ops.metapath_walk([], 8)
    with pytest.raises(ValueError, match="hops"):
        ops.metapath_walk([ap, apt] * 4 + [ap], 8)                           # nine
    with pytest.raises(ValueError, match="CSRGraph"):
        ops.metapath_walk([(ap.rowptr, ap.colidx)], 8)
    with pytest.raises(ValueError, match="columns"):
        ops.metapath_walk([ap, ap], 8)
    with pytest.raises(ValueError, match="walks"):
        ops.metapath_walk([ap, apt], 0)
    with pytest.raises(ValueError, match="walks"):
        ops.metapath_walk([ap, apt], ops.WALK_MAX_WALKS + 1)
    with pytest.raises(ValueError, match="fanout"):
        ops.metapath_walk([ap, apt], 8, 9)
    with pytest.raises(ValueError, match="fanout"):
        ops.metapath_walk([ap, apt], 8, 0)
    with pytest.raises(ValueError, match="seed"):
        ops.metapath_walk([ap, apt], 8, seed=-3)
    with pytest.raises(ValueError, match="square"):
        ops.metapath_walk([ap, pc], 8, diag=True)
    with pytest.raises(ValueError, match="rows"):
        ops.metapath_walk([ap, apt], 8, rows=(2, 5))
    with pytest.raises(ValueError, match="no CPU path"):
        ops.metapath_walk([ap, apt], 8, 4, diag=True, rows=(1, 2))
    with pytest.raises(ValueError, match="no CPU path"):
        ops.metapath_walk([ap, pc], ops.WALK_MAX_WALKS)
    assert (ops.WALK_MAX_HOPS, ops.WALK_MAX_WALKS) == (8, 4096)


def test_abi_declares_the_walk_entry_points():
    from han_amd import _lib
    assert _lib.ABI_VERSION >= 11
    for name in ("han_metapath_walk_count", "han_metapath_walk_fill"):
        assert name in _lib.SIGNATURES


def test_hub_preset_is_declared():
    from han_amd import synth
    assert synth.HETERO["hub-1m"] == dict(P=3_000_000, A=1_000_000, C=4000)
    assert synth.HETERO["pap-3m"] == dict(P=3_000_000, A=1_000_000)
    with pytest.raises(ValueError, match="hub-1m"):
        synth.hetero_relations("hub")
