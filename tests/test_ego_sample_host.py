"""Sampled ego blocks, host side (no GPU): the refusals of ego_block(fanout=, seed=) that come before any device is asked
for, the NumPy reference of the rule (tests/ego_sample_ref.py) against the unsampled reference on the thinned graphs,
the uniformity of the rule, the existence of equal keys, and the bad-argument returns of the han_ego_sample_* entries."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from han_amd import _lib, minibatch
from han_amd.graph import CSRGraph
from tests import ego_block_ref as ref
from tests import ego_sample_ref as sref
from tests.rng_ref import splitmix64

N = 1543


# ---- refusals ----------------------------------------------------------------------------------------------------------
def _cpu_graph(n=6):
    return CSRGraph(torch.arange(n + 1, dtype=torch.int64), torch.arange(n, dtype=torch.int32), n)


@pytest.fixture
def no_library(monkeypatch):
    calls = []

    def load():
        calls.append(1)
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(_lib, "load", load)
    return calls


@pytest.mark.parametrize("fanout", [True, 2.5, np.float32(3.0), "3", (2, False), (2, 1.5)])
def test_fanout_that_is_no_integer_raises(fanout):
    with pytest.raises(ValueError, match="fanout"):
        minibatch.ego_block([_cpu_graph()], [0], hops=2 if isinstance(fanout, tuple) else 1, fanout=fanout)


@pytest.mark.parametrize("fanout,hops", [(0, 1), (-1, 1), ((3, 0), 2), ((3, 3), 1), ((3,), 2), ([], 1), ([4, 4, 4], 2)])
def test_bad_fanout_raises_before_any_library_call(fanout, hops, no_library):
    with pytest.raises(ValueError, match="fanout"):
        minibatch.ego_block([_cpu_graph()], [0], hops=hops, fanout=fanout)
    with pytest.raises(ValueError, match="fanout"):
        minibatch.ego_block([_cpu_graph()], torch.tensor([0]), hops=hops, fanout=fanout)
    assert not no_library


@pytest.mark.parametrize("seed", [1.5, "7", None, True])
def test_seed_that_is_no_integer_raises(seed, no_library):
    with pytest.raises(ValueError, match="seed"):
        minibatch.ego_block([_cpu_graph()], [0], hops=1, fanout=3, seed=seed)
    assert not no_library


@pytest.mark.parametrize("fanout,hops,seed", [(3, 1, 0), ((3, 2), 2, -1), ([5], 1, 2 ** 64 + 3), (np.int64(2), 2, np.int32(4))])
def test_a_good_fanout_gets_as_far_as_the_device_requirement(fanout, hops, seed):
    with pytest.raises(ValueError, match="GPU"):
        minibatch.ego_block([_cpu_graph()], [0], hops=hops, fanout=fanout, seed=seed)


def test_block_seeds_are_splitmix64_of_trainer_seed_and_step():
    for s in (0, 5, -3, 2 ** 64 + 9):
        got = [minibatch.block_seed(s, t) for t in range(4)]
        want = [splitmix64((splitmix64(s & (2 ** 64 - 1)) + t) & (2 ** 64 - 1)) for t in range(4)]
        assert got == want and len(set(got)) == 4
    assert minibatch.block_seed(1, 0) != minibatch.block_seed(2, 0)


# ---- the reference: identity with the unsampled rule on the thinned graphs ---------------------------------------------
@functools.lru_cache(maxsize=None)
def _graph_abc():
    """The graph family of the ego-block structure test, rebuilt here: (a) rows drawn with repeats, unsorted, degrees
    0 .. 1025 and one row adjacent to everybody, (b) a symmetric valued graph, (c) the ring i -> i, i + 1."""
    rng = np.random.default_rng(42)
    rows = [rng.integers(0, N, d) for d in rng.integers(0, 4, N)]
    for i, d in {5: 0, 6: 1, 7: 63, 8: 64, 9: 65, 10: 129, 11: 1025, 0: 65, N - 1: 129, 700: 1025}.items():
        rows[i] = rng.integers(0, N, d)
    rows[12] = rng.permutation(N)
    rows[13] = np.concatenate([rows[9], rows[9][:7]])
    a = ref.from_rows(rows)
    iu, ju = np.triu_indices(N, 1)
    sel = rng.random(iu.size) < 0.01
    adj = np.zeros((N, N), dtype=bool)
    adj[iu[sel], ju[sel]] = adj[ju[sel], iu[sel]] = True
    brow = [np.nonzero(r)[0] for r in adj]
    b = ref.from_rows(brow, [rng.random(len(r)).astype(np.float32) for r in brow])
    c = ref.from_rows([[i, (i + 1) % N] for i in range(N)])
    return a, b, c


@pytest.mark.parametrize("hops,fanout", [(1, 5), (1, (40,)), (2, 3), (2, (7, 3)), (2, (2, 70))])
def test_sampled_reference_is_the_unsampled_reference_on_the_thinned_graphs(hops, fanout):
    graphs = list(_graph_abc())
    rng = np.random.default_rng(7)
    for seeds in (np.array([12]), np.array([N - 1]), rng.permutation(N)[:37], np.arange(N)[::-1]):
        level, sel = sref.sampled_rows(graphs, seeds, hops, fanout, seed=11)
        got = sref.ego_sample_ref(graphs, seeds, hops, fanout, seed=11)
        want = ref.ego_block_ref(sref.thinned(graphs, sel), seeds, hops)
        assert sref.blocks_equal(got, want)
        assert np.array_equal(got["nodes"], np.nonzero(level >= 0)[0])
        fan = sref.fanouts(fanout, hops)
        for p, (rowptr, colidx, _) in enumerate(graphs):           # the rule, row by row
            assert sorted(sel[p]) == np.nonzero((level >= 0) & (level < hops))[0].tolist()
            for v, pos in sel[p].items():
                row = colidx[rowptr[v]:rowptr[v + 1]]
                d, f = int((row != v).sum()), fan[level[v]]
                assert np.all(np.diff(pos) > 0) and pos.size == min(d, f) + (row.size - d)
                assert np.all(np.isin(np.nonzero(row == v)[0], pos))
    whole = sref.ego_sample_ref(graphs, np.array([3, 12]), 2, 10 ** 6, seed=1)      # no row is longer: nothing is cut
    assert sref.blocks_equal(whole, ref.ego_block_ref(graphs, np.array([3, 12]), 2))


def test_another_seed_or_graph_number_draws_another_subset():
    cols = np.arange(1, 101)
    a = sref.select_positions(cols, 0, 0, 10, seed=1)
    assert np.array_equal(a, sref.select_positions(cols, 0, 0, 10, seed=1))
    assert np.array_equal(a, sref.select_positions(cols, 0, 0, 10, seed=1 + 2 ** 64))     # the seed is taken mod 2^64
    for other in (sref.select_positions(cols, 0, 0, 10, seed=2), sref.select_positions(cols, 0, 1, 10, seed=1),
                  sref.select_positions(cols + 1, 1, 0, 10, seed=1)):
        assert other.size == 10 and not np.array_equal(a, other)


# ---- uniformity of the rule ----------------------------------------------------------------------------------------------
def _max_z(counts, trials, d, f):
    q = f / d
    return float(np.abs(counts - trials * q).max() / np.sqrt(trials * q * (1 - q)))


@pytest.mark.parametrize("d,f,v,p", [(20, 5, 7, 0), (64, 10, 0, 0), (200, 25, 999999, 3)])
def test_every_position_is_kept_equally_often_over_seeds(d, f, v, p):
    """4 000 seeds splitmix64(1000 + t): inclusion counts within 5 sigma of T f / d (binomial sigma; a cap, not a fit)."""
    cols = (v + 1 + np.arange(d)) % 2000000
    counts = np.zeros(d)
    for t in range(4000):
        counts[sref.select_positions(cols, v, p, f, splitmix64(1000 + t))] += 1
    z = _max_z(counts, 4000, d, f)
    print(f"d {d} f {f} v {v} p {p}: max |z| {z:.2f}")
    assert counts.sum() == 4000 * f and z < 5.0


def test_every_position_is_kept_equally_often_over_rows():
    counts = np.zeros(20)
    for v in range(4000):
        counts[sref.select_positions((v + 1 + np.arange(20)) % 4000, v, 0, 5, 12345)] += 1
    z = _max_z(counts, 4000, 20, 5)
    print(f"over rows: max |z| {z:.2f}")
    assert z < 5.0


def test_equal_keys_exist_in_a_long_row_and_not_in_a_short_one():
    f, pairs = sref.tie_fanout(99, 0, 5, 10 ** 6)
    assert pairs == 105 and f is not None and 1 <= f < 10 ** 6
    assert sref.tie_fanout(99, 0, 5, 3000) == (None, 0)
    x = sref.row_keys(99, 0, 5, 10 ** 6)
    order = np.lexsort((np.arange(x.size), x))
    assert x[order[f - 1]] == x[order[f]] and order[f - 1] < order[f]       # the cut falls between two equal keys
    pos = sref.select_positions(np.full(10 ** 6, 7), 5, 0, f, 99)
    assert np.array_equal(pos, np.sort(order[:f]))


# ---- C ABI -------------------------------------------------------------------------------------------------------------
def test_sample_entry_points_check_their_arguments_before_any_launch():
    assert _lib.ABI_VERSION == 15
    assert {"han_ego_sample_expand", "han_ego_sample_count", "han_ego_sample_fill"} <= set(_lib.SIGNATURES)
    lib = _lib.load()
    assert lib.han_abi_version() == 15
    rp = (ctypes.c_int64 * 5)(0, 1, 2, 3, 4)            # a host array stands in: nothing is launched on these paths
    p = ctypes.cast(rp, ctypes.c_void_p)
    no_long = (0, 0, None)

    def expand(rowptr=p, colidx=None, n=4, h=0, fanout=3, graph=0, long=no_long, level=p, thr=p, need=p, kept=p):
        return lib.han_ego_sample_expand(rowptr, colidx, n, h, fanout, 7, graph, *long, level, thr, need, kept, None)
    assert expand() == 0                                 # no entries (NULL colidx): nothing to do
    assert expand(n=0) == 0
    for bad in (dict(rowptr=None), dict(level=None), dict(thr=None), dict(need=None), dict(kept=None), dict(n=-1),
                dict(n=2 ** 31), dict(h=-1), dict(fanout=0), dict(fanout=-5), dict(graph=-1), dict(long=(8, 1, None)),
                dict(long=(0, 1, p)), dict(long=(8, -1, p))):
        assert expand(**bad) == -1, bad

    def count(rows=p, level=p, hops=1, kept=p, n_in=4, n_out=4, counts=p):
        return lib.han_ego_sample_count(rows, level, hops, kept, n_in, n_out, counts, None)
    assert count(n_out=0, rows=None, counts=None) == 0
    for bad in (dict(rows=None), dict(level=None), dict(kept=None), dict(counts=None), dict(hops=0), dict(n_in=-1),
                dict(n_out=-1)):
        assert count(**bad) == -1, bad

    def fill(rowptr=p, rows=p, level=p, hops=1, local=p, n_in=4, n_out=4, graph=0, long=no_long, thr=p, need=p,
             out_rowptr=p, out_colidx=p):
        return lib.han_ego_sample_fill(rowptr, p, None, rows, level, hops, local, n_in, n_out, 7, graph, *long, thr,
                                       need, out_rowptr, out_colidx, None, None)
    assert fill(n_out=0, rows=None, out_rowptr=None, out_colidx=None) == 0
    for bad in (dict(rowptr=None), dict(rows=None), dict(level=None), dict(local=None), dict(thr=None), dict(need=None),
                dict(out_rowptr=None), dict(out_colidx=None), dict(hops=0), dict(n_in=-1), dict(n_in=2 ** 31),
                dict(n_out=-1), dict(n_out=2 ** 31), dict(graph=-1), dict(long=(8, 1, None)), dict(long=(0, 2, p))):
        assert fill(**bad) == -1, bad
