"""Ego blocks, host side (no GPU): the NumPy reference the GPU tests compare the kernels with (tests/ego_block_ref.py)
against the dense brute force, the identity block, the batch iterator of MiniBatchTrainer, and every ValueError of
minibatch.ego_block that is raised before a GPU is asked for."""
import numpy as np
import pytest
import torch

from han_amd import minibatch
from han_amd.graph import CSRGraph
from tests import ego_block_ref as ref


def _random_graphs(seed, n, p, values=True):
    """p directed graphs over n nodes: rows of 0 .. 4 entries drawn with repeats, unsorted; every other one valued."""
    rng = np.random.default_rng(seed)
    out = []
    for q in range(p):
        rows = [rng.integers(0, n, d) for d in rng.integers(0, 5, n)]
        vals = [rng.random(len(r)).astype(np.float32) for r in rows] if values and q % 2 == 0 else None
        out.append(ref.from_rows(rows, vals))
    return out


@pytest.mark.parametrize("hops", [1, 2, 3])
@pytest.mark.parametrize("seed,n,p,b", [(0, 40, 1, 1), (1, 97, 3, 5), (2, 150, 2, 20)])
def test_reference_matches_the_dense_brute_force(seed, n, p, b, hops):
    graphs = _random_graphs(seed, n, p)
    seeds = np.random.default_rng(seed + 10).permutation(n)[:b]
    blk = ref.ego_block_ref(graphs, seeds, hops)
    level = ref.brute_force_levels(graphs, seeds, hops)
    assert np.array_equal(blk["nodes"], np.nonzero(level >= 0)[0])
    assert np.array_equal(blk["level"], level[blk["nodes"]])
    assert np.array_equal(blk["nodes"][blk["seed_pos"]], seeds)
    assert 0 < blk["nodes"].size < n or hops > 1          # the cases are not all the whole graph
    for (rowptr, colidx, values), (brp, bci, bv) in zip(graphs, blk["graphs"]):
        assert (values is None) == (bv is None)
        for r, v in enumerate(blk["nodes"]):
            got = bci[brp[r]:brp[r + 1]]
            if blk["level"][r] < hops:                     # kept whole, in stored order, every neighbour inside
                want = colidx[rowptr[v]:rowptr[v + 1]]
                assert np.array_equal(blk["nodes"][got], want)
                if values is not None:
                    assert np.array_equal(bv[brp[r]:brp[r + 1]], values[rowptr[v]:rowptr[v + 1]])
            else:
                assert got.tolist() == [r]
                if values is not None:
                    assert bv[brp[r]:brp[r + 1]].tolist() == [1.0]


@pytest.mark.parametrize("hops", [1, 2])
def test_block_of_all_nodes_is_the_input_graph(hops):
    graphs = _random_graphs(5, 64, 3)
    blk = ref.ego_block_ref(graphs, np.arange(64)[::-1], hops)
    assert np.array_equal(blk["nodes"], np.arange(64)) and not blk["level"].any()
    assert np.array_equal(blk["seed_pos"], np.arange(64)[::-1])
    for (rowptr, colidx, values), (brp, bci, bv) in zip(graphs, blk["graphs"]):
        assert np.array_equal(brp, rowptr) and np.array_equal(bci, colidx)
        assert (values is None and bv is None) or np.array_equal(bv, values)


def test_ring_adds_one_node_per_seed_and_hop():
    n = 50
    ring = ref.from_rows([[i, (i + 1) % n] for i in range(n)])
    for hops in (1, 2, 3):
        blk = ref.ego_block_ref([ring], [7, 30, n - 1], hops)
        assert blk["nodes"].size == 3 * (hops + 1)
        assert sorted(blk["nodes"].tolist()) == sorted((s + k) % n for s in (7, 30, n - 1) for k in range(hops + 1))


# ---- the batch iterator ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_train,batch", [(10, 3), (64, 64), (65, 64), (7, 100), (1, 1)])
def test_epoch_batches_visit_every_training_node_once(n_train, batch):
    ids = np.random.default_rng(3).permutation(1000)[:n_train]
    bs = minibatch.epoch_batches(ids, batch, seed=5, epoch=0)
    assert len(bs) == -(-n_train // batch)
    assert all(b.size == batch for b in bs[:-1]) and bs[-1].size == n_train - batch * (len(bs) - 1)     # short last batch kept
    assert sorted(np.concatenate(bs).tolist()) == sorted(ids.tolist())


def test_epoch_batches_are_a_function_of_seed_and_epoch():
    ids = np.arange(100, 400)
    a = [minibatch.epoch_batches(ids, 32, seed=9, epoch=e) for e in range(3)]
    b = [minibatch.epoch_batches(ids, 32, seed=9, epoch=e) for e in range(3)]
    for x, y in zip(a, b):
        assert len(x) == len(y) and all(np.array_equal(u, v) for u, v in zip(x, y))
    assert not np.array_equal(np.concatenate(a[0]), np.concatenate(a[1]))            # a new order every epoch
    other = minibatch.epoch_batches(ids, 32, seed=10, epoch=0)
    assert not np.array_equal(np.concatenate(a[0]), np.concatenate(other))
    assert not np.array_equal(np.concatenate(a[0]), ids)                               # and not the given one
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError):
            minibatch.epoch_batches(ids, bad, 0, 0)


# ---- errors ----------------------------------------------------------------------------------------------------------
def _cpu_graph(n=6, n_cols=None, row_base=0):
    return CSRGraph(torch.arange(n + 1, dtype=torch.int64), (torch.arange(n, dtype=torch.int32) % (n_cols or n)),
                    n_cols, row_base=row_base)


@pytest.mark.parametrize("seeds,match", [([1, 1], "repeated"), ([0, 6], "outside"), ([-1], "outside"), ([], "empty"),
                                         ([[0, 1]], "1-D"), ([0.5], "integer")])
def test_bad_seeds_raise_before_any_device_is_touched(seeds, match):
    with pytest.raises(ValueError, match=match):
        minibatch.ego_block([_cpu_graph()], np.asarray(seeds), hops=1)


def test_bad_seed_tensors_raise():
    with pytest.raises(ValueError, match="empty"):
        minibatch.ego_block([_cpu_graph()], torch.zeros(0, dtype=torch.int64))
    with pytest.raises(ValueError, match="int32 / int64"):
        minibatch.ego_block([_cpu_graph()], torch.zeros(2, dtype=torch.float32))
    with pytest.raises(ValueError, match="1-D"):
        minibatch.ego_block([_cpu_graph()], torch.zeros((2, 2), dtype=torch.int64))


@pytest.mark.parametrize("hops", [0, -1, 1.5, True])
def test_bad_hops_raise(hops):
    with pytest.raises(ValueError, match="hops"):
        minibatch.ego_block([_cpu_graph()], [0], hops=hops)


def test_bad_graphs_raise():
    with pytest.raises(ValueError, match="square"):
        minibatch.ego_block([_cpu_graph(6, n_cols=9)], [0])
    with pytest.raises(ValueError, match="nodes"):
        minibatch.ego_block([_cpu_graph(6), _cpu_graph(7)], [0])
    with pytest.raises(ValueError, match="row_base"):
        minibatch.ego_block([_cpu_graph(6, row_base=2)], [0])
    with pytest.raises(ValueError, match="no graphs"):
        minibatch.ego_block([], [0])
    with pytest.raises(ValueError, match="CSRGraph"):
        minibatch.ego_block([(np.zeros(2), np.zeros(0))], [0])


def test_there_is_no_cpu_path():
    with pytest.raises(ValueError, match="GPU"):
        minibatch.ego_block([_cpu_graph()], [0, 3])
    with pytest.raises(ValueError, match="GPU"):
        minibatch.ego_block([_cpu_graph()], torch.tensor([0, 3]))
    from han_amd.features import SparseFeatures
    with pytest.raises(ValueError, match="GPU"):
        SparseFeatures.from_dense(torch.eye(4)).take([0, 1])


def test_abi_14_declares_the_ego_entry_points_and_checks_arguments_before_any_launch():
    from han_amd import _lib
    assert _lib.ABI_VERSION >= 14
    assert {"han_ego_expand", "han_ego_count", "han_ego_fill"} <= set(_lib.SIGNATURES)
    lib = _lib.load()
    none6 = (0, 0, None, None, None, None)
    assert lib.han_ego_expand(None, None, 4, 0, *none6, None, None) == -1                      # NULL rowptr / level
    assert lib.han_ego_count(None, None, None, 1, 4, 4, None, None) == -1
    assert lib.han_ego_fill(None, None, None, None, None, 1, None, 4, 4, 4, *none6, None, None, None, None) == -1
    # the remaining checks need a non-NULL rowptr: a host array stands in, nothing is launched on these paths
    import ctypes
    rp = (ctypes.c_int64 * 5)(0, 1, 2, 3, 4)
    p = ctypes.cast(rp, ctypes.c_void_p)
    assert lib.han_ego_expand(p, None, -1, 0, *none6, p, None) == -1                           # negative size
    assert lib.han_ego_expand(p, None, 2 ** 31, 0, *none6, p, None) == -1                      # n beyond int32
    assert lib.han_ego_expand(p, None, 4, -1, *none6, p, None) == -1                           # negative level
    assert lib.han_ego_expand(p, None, 4, 0, 8, 1, None, None, None, None, p, None) == -1      # chunk table without arrays
    assert lib.han_ego_expand(p, None, 4, 0, 0, 1, p, p, p, p, p, None) == -1                  # ... without split_deg
    assert lib.han_ego_expand(p, None, 0, 0, *none6, p, None) == 0                             # no rows: nothing to do
    assert lib.han_ego_expand(p, None, 4, 0, *none6, p, None) == 0                             # no entries (NULL colidx)
    assert lib.han_ego_count(p, p, p, 0, 4, 4, p, None) == -1                                  # hops < 1 beside levels
    assert lib.han_ego_count(p, None, None, 1, 4, 0, None, None) == 0                          # no output rows
    assert lib.han_ego_count(p, None, None, 1, 4, 4, p, None) == -1                            # NULL rows
    assert lib.han_ego_fill(p, p, None, p, None, 1, None, 4, 4, 4, 8, 1, p, p, p, p, p, p, None, None) == -1   # chunks, no map
    assert lib.han_ego_fill(p, p, None, p, None, 1, None, 4, 2 ** 31, 4, *none6, p, p, None, None) == -1
    assert lib.han_ego_fill(p, p, None, p, None, 1, None, 4, 4, 0, *none6, None, None, None, None) == 0
    assert lib.han_ego_fill(p, p, None, p, None, 1, None, 4, 4, 4, *none6, None, p, None, None) == -1          # NULL out_rowptr
