"""Sampled ego blocks on the GPU (minibatch.ego_block(fanout=, seed=), csrc/ego_block.hip): (1) the block structure by
exact equality with the NumPy reference (tests/ego_sample_ref.py), (2) identity with the unsampled rule on the thinned
graphs G', (3) limits, (4) exact ties in a row of 10^6 entries, (5) inclusion statistics, (6) model outputs against
full-graph inference on G', (7) the trainer.  Bounds: structure is exact; model outputs 2e-4 (two GPU results each
within 1e-4 of the oracle, as tests/test_ego_block_gpu.py compares block and full graph); statistics 5 sigma."""
import functools

import numpy as np
import pytest
import torch

from han_amd import minibatch
from han_amd.graph import CSRGraph
from tests import ego_block_ref as ref
from tests import ego_sample_ref as sref
from tests.helpers import build_model, gpu_inputs, make_problem

pytestmark = pytest.mark.gpu

N = 1500
F0, F1 = 7, 3
# non-self degrees around every boundary of the fan-outs 7 and 3, of the wave (64) and of CHUNK (1024), one row of
# about 3 000 (several radix rounds in the workgroup kernel); the id of such a row is 10 (index + 1)
DEGREES = (0, 1, F1 - 1, F1, F1 + 1, F0 - 1, F0, F0 + 1, 63, 64, 65, 1023, 1024, 1025, 3001, 40, 200)
SPECIAL = {10 * (j + 1): (d, j % 3) for j, d in enumerate(DEGREES)}          # row -> (degree off the diagonal, self entries)
SPECIAL[300] = (0, 3)                                                        # a row of self entries only
SPECIAL[N - 1] = (65, 1)


def _with_selfs(rng, v, d, n_self):
    """d columns != v drawn with repeats, unsorted, and n_self entries v at random positions."""
    cols = rng.integers(0, N - 1, d)
    cols = cols + (cols >= v)
    return rng.permutation(np.concatenate([cols, np.full(n_self, v)])).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _graphs():
    """(a) no values, repeated entries, unsorted rows, the special rows; (b) valued, symmetric, a self entry on every
    third row, two rows beyond both fan-outs; (c) the ring i -> i, i + 1: the special row v is one hop from v - 1."""
    rng = np.random.default_rng(2024)
    rows = [_with_selfs(rng, v, d, 0) for v, d in enumerate(rng.integers(0, 4, N))]
    for v, (d, n_self) in SPECIAL.items():
        rows[v] = _with_selfs(rng, v, d, n_self)
    a = ref.from_rows(rows)
    iu, ju = np.triu_indices(N, 1)
    sel = rng.random(iu.size) < 0.004
    adj = np.zeros((N, N), dtype=bool)
    adj[iu[sel], ju[sel]] = adj[ju[sel], iu[sel]] = True
    adj[np.arange(0, N, 3), np.arange(0, N, 3)] = True
    adj[20, ::5] = adj[::5, 20] = True
    brow = [np.nonzero(r)[0] for r in adj]
    b = ref.from_rows(brow, [rng.random(len(r)).astype(np.float32) for r in brow])
    c = ref.from_rows([[i, (i + 1) % N] for i in range(N)])
    return a, b, c


@functools.lru_cache(maxsize=None)
def _seed_sets():
    rng = np.random.default_rng(7)
    before = np.array(sorted(SPECIAL)) - 1                        # their ring entry puts every special row at level 1
    some = np.concatenate([before, [30, 140]])                    # ... and two of them are seeds themselves
    rest = np.setdiff1d(np.arange(N), np.concatenate([some, sorted(SPECIAL)]))
    some = np.concatenate([some, rng.permutation(rest)[:37 - some.size]])          # 37 seeds
    return {"single": np.array([150]), "last": np.array([N - 1]), "some": rng.permutation(some),
            "all": np.arange(N)[::-1].copy()}


CASES = {"hops1": (1, F0), "hops2": (2, (F0, F1)), "hops2_swapped": (2, (F1, F0))}
SEED = 2 ** 63 + 77


@functools.lru_cache(maxsize=None)
def _reference(case, sset):
    """Computed once per case, shared by the chunked and the unchunked run and by the identity test; read only."""
    hops, fanout = CASES[case]
    return sref.ego_sample_ref(list(_graphs()), _seed_sets()[sset], hops, fanout, SEED)


def _to_gpu(g, dev):
    rowptr, colidx, values = g
    return CSRGraph(torch.as_tensor(rowptr).to(dev), torch.as_tensor(colidx).to(dev), rowptr.size - 1,
                    values=torch.as_tensor(values).to(dev) if values is not None else None)


def _to_host(blk):
    return dict(nodes=blk.nodes.cpu().numpy(), level=blk.level.cpu().numpy(), seed_pos=blk.seed_pos.cpu().numpy(),
                graphs=[(g.rowptr.cpu().numpy(), g.colidx.cpu().numpy(),
                         g.values.cpu().numpy() if g.values is not None else None) for g in blk.graphs])


def _bit_equal(a, b):
    return sref.blocks_equal(_to_host(a), _to_host(b))


# ---- 1. structure ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [None, 100], ids=["chunk1024", "chunk100"])
@pytest.mark.parametrize("case", list(CASES))
def test_sampled_block_structure_equals_the_reference(dev, case, chunk, monkeypatch):
    """nodes, level, seed_pos and every block graph's rowptr / colidx / values for the four seed sets, host and device
    seeds.  chunk1024: the rows of 1025 and 3001 entries go through the workgroup kernels; chunk100: those from 200 on."""
    if chunk is not None:
        monkeypatch.setattr(minibatch, "CHUNK", chunk)
    hops, fanout = CASES[case]
    graphs = [_to_gpu(g, dev) for g in _graphs()]
    for k, (sset, seeds) in enumerate(_seed_sets().items()):
        want = _reference(case, sset)
        given = (seeds, torch.as_tensor(seeds).to(dev), torch.as_tensor(seeds).to(dev, torch.int32))[(k + hops) % 3]
        blk = minibatch.ego_block(graphs, given, hops, fanout=fanout, seed=SEED)
        assert blk.nodes.dtype == torch.int64 and blk.level.dtype == torch.int32 and blk.seed_pos.dtype == torch.int64
        assert blk.n == N
        got = _to_host(blk)
        for key in ("nodes", "level", "seed_pos"):
            assert np.array_equal(got[key], want[key]), (sset, key)
        for p, ((rp, ci, va), (rq, cj, vb)) in enumerate(zip(got["graphs"], want["graphs"])):
            assert np.array_equal(rp, rq), (sset, p)
            assert np.array_equal(ci, cj), (sset, p)
            assert (va is None) == (vb is None) and (va is None or np.array_equal(va, vb)), (sset, p)
        for g in blk.graphs:
            g.validate()
    assert graphs[0].row_split(chunk or 1024, chunk or 1024)["n_long"] >= (2 if chunk is None else 5)    # they did run
    if case != "hops1":                                    # the special rows were sampled at level 1 as well
        lv = dict(zip(_reference(case, "some")["nodes"].tolist(), _reference(case, "some")["level"].tolist()))
        assert sum(lv[v] == 1 for v in SPECIAL) >= len(SPECIAL) - 3


# ---- 2. identity with the unsampled rule -------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_sampled_block_is_the_unsampled_block_of_the_thinned_graphs(dev, case):
    hops, fanout = CASES[case]
    host = list(_graphs())
    graphs = [_to_gpu(g, dev) for g in host]
    for sset in ("some", "all"):
        seeds = _seed_sets()[sset]
        thin = [_to_gpu(g, dev) for g in sref.thinned_graphs(host, seeds, hops, fanout, SEED)]
        assert sum(g.nnz for g in thin) < sum(g.nnz for g in graphs)
        assert _bit_equal(minibatch.ego_block(graphs, seeds, hops, fanout=fanout, seed=SEED),
                          minibatch.ego_block(thin, seeds, hops)), sset


# ---- 3. limits -----------------------------------------------------------------------------------------------------------
def test_limits_of_the_rule(dev):
    host = list(_graphs())
    graphs = [_to_gpu(g, dev) for g in host]
    seeds = _seed_sets()["some"]
    max_deg = max(int(np.diff(g[0]).max()) for g in host)
    for hops in (1, 2):                                    # nothing to cut: the unsampled block, bit for bit
        plain = minibatch.ego_block(graphs, seeds, hops)
        assert _bit_equal(minibatch.ego_block(graphs, seeds, hops, fanout=max_deg, seed=5), plain)
        assert _bit_equal(minibatch.ego_block(graphs, seeds, hops, fanout=[2 ** 31 - 1] * hops, seed=6), plain)
    everyone = np.arange(N)
    a = minibatch.ego_block(graphs, everyone, 1, fanout=F0, seed=1)
    assert _bit_equal(a, minibatch.ego_block(graphs, everyone, 1, fanout=F0, seed=1))
    assert _bit_equal(a, minibatch.ego_block(graphs, everyone, 1, fanout=(F0,), seed=1 + 2 ** 64))      # mod 2^64
    b = minibatch.ego_block(graphs, everyone, 1, fanout=F0, seed=2)
    assert torch.equal(a.nodes, b.nodes) and torch.equal(a.nodes.cpu(), torch.arange(N))       # all seeds: local == global
    for p, (rowptr, colidx, values) in enumerate(host):
        ga, gb = _to_host(a)["graphs"][p], _to_host(b)["graphs"][p]
        differ = 0
        for v in range(N):
            row = colidx[rowptr[v]:rowptr[v + 1]]
            got = ga[1][ga[0][v]:ga[0][v + 1]]
            d = int((row != v).sum())
            assert got.size == min(d, F0) + (row.size - d), (p, v)       # exactly min(d, f) + the self entries
            it = iter(row.tolist())
            assert all(c in it for c in got.tolist()), (p, v)            # a subsequence of the stored row
            assert int((got == v).sum()) == row.size - d
            other = gb[1][gb[0][v]:gb[0][v + 1]]
            if d > F0:
                differ += not np.array_equal(got, other)
            else:
                assert np.array_equal(got, row) and np.array_equal(other, row)
                if p == 0 and v == 150:
                    assert d == 3001 and not np.array_equal(got, other)  # another seed, another subset
        n_cut = sum(int((colidx[rowptr[v]:rowptr[v + 1]] != v).sum()) > F0 for v in range(N))
        assert 2 * differ >= n_cut, (p, differ, n_cut)       # (a row of 8 keeps the same 7 once in 8 times)


# ---- 4. exact ties -------------------------------------------------------------------------------------------------------
def test_a_cut_between_two_equal_keys_goes_to_the_smaller_position(dev):
    """Row 5 of a graph of 2 000 nodes holds 10^6 entries (repeats, none of them 5); at seed 99 its keys hold 105
    equal pairs, and f is chosen so that the f-th and (f + 1)-th smallest (key, position) share their key."""
    n, d = 2000, 10 ** 6
    f, pairs = sref.tie_fanout(99, 0, 5, d)
    assert pairs == 105
    rng = np.random.default_rng(3)
    cols = rng.integers(0, n - 1, d)
    cols = (cols + (cols >= 5)).astype(np.int32)
    rows = [np.zeros(0, np.int32)] * n
    rows[5] = cols
    host = ref.from_rows(rows)
    want = sref.ego_sample_ref([host], np.array([5]), 1, f, 99)
    blk = minibatch.ego_block([_to_gpu(host, dev)], [5], 1, fanout=f, seed=99)
    assert sref.blocks_equal(_to_host(blk), want)
    r = int(blk.seed_pos[0])
    assert int(blk.graphs[0].rowptr[r + 1] - blk.graphs[0].rowptr[r]) == f
    again = minibatch.ego_block([_to_gpu(host, dev)], [5], 1, fanout=f + 1, seed=99)     # one more takes the other of the pair
    assert sref.blocks_equal(_to_host(again), sref.ego_sample_ref([host], np.array([5]), 1, f + 1, 99))


# ---- 5. statistics ---------------------------------------------------------------------------------------------------------
def test_every_position_is_kept_equally_often_on_the_device(dev):
    """4 000 rows of 20 entries, fan-out 5, one seed: the inclusion count of every stored position over the rows is
    within 5 binomial sigma of 1 000."""
    n, d, f = 4000, 20, 5
    host = ref.from_rows([(v + 1 + np.arange(d)) % n for v in range(n)])
    blk = minibatch.ego_block([_to_gpu(host, dev)], np.arange(n), 1, fanout=f, seed=12345)
    g = blk.graphs[0]
    assert torch.equal(g.rowptr.cpu(), torch.arange(n + 1) * f)
    k = (g.colidx.cpu().numpy().reshape(n, f) - np.arange(n)[:, None] - 1) % n
    assert k.max() < d and np.all(np.diff(k, axis=1) > 0)
    counts = np.bincount(k.ravel(), minlength=d)
    z = float(np.abs(counts - n * f / d).max() / np.sqrt(n * (f / d) * (1 - f / d)))
    print(f"inclusion counts {counts.tolist()}: max |z| {z:.2f}")
    assert z < 5.0


# ---- 6. model ----------------------------------------------------------------------------------------------------------------
MODELS = {"one_layer": (dict(), 4), "two_layers_residual": (dict(hid_units=[8, 16], n_heads=(8, 4, 1), residual=True), (4, 3))}


def _infer(model, kw, x, graphs):
    with torch.no_grad():
        lg, fe, att = model.inference([x] * 2, 3, graphs[0].n_rows, False, 0.0, 0.0, graphs, kw.get("hid_units", [8]),
                                      list(kw.get("n_heads", (8, 1))), residual=kw.get("residual", False))
    return lg[0], fe, att


@pytest.mark.parametrize("name", list(MODELS))
def test_sampled_block_outputs_are_full_graph_inference_on_the_thinned_graphs(dev, name):
    kw, fanout = MODELS[name]
    prob = make_problem(31, 300, 24, 2, 3, (0.02, 0.1), **kw)
    model, _ = build_model(prob, dev)
    x, graphs = gpu_inputs(prob, dev)
    hops = 1 + len(model.extra)
    rng = np.random.default_rng(5)
    seeds = rng.permutation(np.concatenate([[0, 1, 2], 3 + rng.permutation(297)[:37]]))
    assert all(g.values is None for g in graphs)
    host = [(g.rowptr.cpu().numpy(), g.colidx.cpu().numpy(), None) for g in graphs]
    thin = sref.thinned_graphs(host, seeds, hops, fanout, 21)
    assert sum(g[1].size for g in thin) < sum(g[1].size for g in host)
    blk = minibatch.ego_block(graphs, seeds, hops, fanout=fanout, seed=21)
    got = _infer(model, kw, blk.take(x), blk.graphs)
    full = _infer(model, kw, x, [_to_gpu(g, dev) for g in thin])
    for g, f, what in zip(got, full, ("logits", "final_embed", "att_val")):
        err = float((g[blk.seed_pos] - f[torch.as_tensor(seeds).to(dev)]).abs().max())
        print(f"{name} {what}: sampled block vs full graph on G': max abs difference {err:.3e} (bound 2e-4)")
        assert err < 2e-4, (what, err)


# ---- 7. trainer ----------------------------------------------------------------------------------------------------------------
def test_trainer_with_a_fanout(dev):
    prob = make_problem(11, 80, 16, 2, 3, [0.05, 0.4])
    x, graphs = gpu_inputs(prob, dev)
    labels = torch.tensor(prob["labels"], dtype=torch.int32, device=dev)
    tm = torch.tensor(prob["mask"].astype(np.uint8))
    max_deg = max(int(g.degrees().max()) for g in graphs)
    assert max_deg > 5

    def run(fanout, seed=4):
        model, _ = build_model(prob, dev)
        tr = minibatch.MiniBatchTrainer(model, [x] * 2, graphs, labels, tm, batch_size=12, attn_drop=0.6, ffd_drop=0.6,
                                        seed=seed, fanout=fanout)
        for b in tr.batches()[:3]:
            tr.train_step(b)
        assert tr.steps_done == 3
        return model.flat.detach().clone(), model

    (a, model), (b, _), (c, _) = run((5,)), run((5,)), run((5,), seed=5)
    assert torch.isfinite(a).all() and torch.equal(a, b) and not torch.equal(a, c)
    (whole, _), (wide, _) = run(None), run(max_deg)
    assert torch.equal(whole, wide)                         # nothing to cut: bit-equal, dropout included
    assert not torch.equal(whole, a)
    rows = np.array([7, 3, 3, 79, 0])
    out = minibatch.predict(model, [x] * 2, graphs, rows=rows, batch_size=2, fanout=5, seed=9)
    exact = minibatch.predict(model, [x] * 2, graphs, rows=rows, batch_size=2)
    for o, e in zip(out, exact):
        assert o.shape == e.shape and torch.isfinite(o).all()
        assert torch.equal(o[1], o[2])                      # the repeated row
    assert torch.equal(minibatch.predict(model, [x] * 2, graphs, rows=rows, batch_size=2, fanout=max_deg)[0], exact[0])
    with pytest.raises(ValueError, match="fanout"):
        minibatch.predict(model, [x] * 2, graphs, rows=rows, fanout=(5, 5))
