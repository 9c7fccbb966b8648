"""Ego blocks on the GPU (han_amd/minibatch.py, csrc/ego_block.hip): (1) the block structure by exact equality with the
NumPy reference, (2) forward parity of block rows with the float64 oracle on the FULL graph, (3) gradient parity,
(4) MiniBatchTrainer against HANTrainer, (5) learning on the planted-partition task.  Bounds are the suite's own for
the same quantities (tests/test_gpu_parity.py): 1e-4 absolute on model outputs against the oracle, 2e-3 relative on
gradients, 2e-4 on parameters after three steps; two GPU results that are each within 1e-4 of the oracle are compared
within 2e-4."""
import functools

import numpy as np
import pytest
import torch

from han_amd import SparseFeatures, minibatch, ops
from han_amd.graph import CSRGraph
from oracle import han_oracle as ho
from oracle import han_oracle_torch as ht
from tests import ego_block_ref as ref
from tests.helpers import build_model, gpu_inputs, make_problem, rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-4
GTOL = 2e-3
N = 1543


# ---- 1. structure ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _graph_abc():
    """The three raw graphs of the structure test, as (rowptr, colidx, values) NumPy triples."""
    rng = np.random.default_rng(42)
    rows = [rng.integers(0, N, d) for d in rng.integers(0, 4, N)]                 # drawn with repeats, unsorted
    for i, d in {5: 0, 6: 1, 7: 63, 8: 64, 9: 65, 10: 129, 11: 1025, 0: 65, N - 1: 129, 700: 1025}.items():
        rows[i] = rng.integers(0, N, d)
    rows[12] = rng.permutation(N)                                                 # adjacent to every node, unsorted
    rows[13] = np.concatenate([rows[9], rows[9][:7]])                             # repeated entries for sure
    a = ref.from_rows(rows)
    iu, ju = np.triu_indices(N, 1)
    sel = rng.random(iu.size) < 0.01
    adj = np.zeros((N, N), dtype=bool)
    adj[iu[sel], ju[sel]] = adj[ju[sel], iu[sel]] = True
    brow = [np.nonzero(r)[0] for r in adj]
    b = ref.from_rows(brow, [rng.random(len(r)).astype(np.float32) for r in brow])
    c = ref.from_rows([[i, (i + 1) % N] for i in range(N)])
    return a, b, c


GRAPH_SETS = {"ring": (2,), "abc": (0, 1, 2)}


@functools.lru_cache(maxsize=None)
def _seed_sets():
    rng = np.random.default_rng(7)
    some = np.concatenate([[0, N - 1], 1 + rng.permutation(N - 2)[:35]])
    return {"first": np.array([0]), "last": np.array([N - 1]), "some": rng.permutation(some),
            "all": np.arange(N)[::-1].copy()}


@functools.lru_cache(maxsize=None)
def _reference(gset, sset, hops):
    """Computed once per case, shared by the chunked and the unchunked run; read only."""
    graphs = [_graph_abc()[i] for i in GRAPH_SETS[gset]]
    return ref.ego_block_ref(graphs, _seed_sets()[sset], hops)


def _to_gpu(g, dev):
    rowptr, colidx, values = g
    return CSRGraph(torch.as_tensor(rowptr).to(dev), torch.as_tensor(colidx).to(dev), rowptr.size - 1,
                    values=torch.as_tensor(values).to(dev) if values is not None else None)


def _assert_block_equals(blk, want):
    assert blk.nodes.dtype == torch.int64 and blk.level.dtype == torch.int32 and blk.seed_pos.dtype == torch.int64
    assert np.array_equal(blk.nodes.cpu().numpy(), want["nodes"])
    assert np.array_equal(blk.level.cpu().numpy(), want["level"])
    assert np.array_equal(blk.seed_pos.cpu().numpy(), want["seed_pos"])
    assert len(blk.graphs) == len(want["graphs"])
    for g, (rowptr, colidx, values) in zip(blk.graphs, want["graphs"]):
        assert g.n_rows == g.n_cols == want["nodes"].size
        assert np.array_equal(g.rowptr.cpu().numpy(), rowptr)
        assert np.array_equal(g.colidx.cpu().numpy(), colidx)
        assert (g.values is None) == (values is None)
        if values is not None:
            assert np.array_equal(g.values.cpu().numpy(), values)
        g.validate()


def _bit_equal(a, b):
    same = torch.equal(a.nodes, b.nodes) and torch.equal(a.level, b.level) and torch.equal(a.seed_pos, b.seed_pos)
    for g, h in zip(a.graphs, b.graphs):
        same = same and torch.equal(g.rowptr, h.rowptr) and torch.equal(g.colidx, h.colidx)
        same = same and ((g.values is None and h.values is None) or torch.equal(g.values, h.values))
    return same


@pytest.mark.parametrize("chunk", [None, 100], ids=["chunk1024", "chunk100"])
@pytest.mark.parametrize("hops", [1, 2, 3])
@pytest.mark.parametrize("gset", ["ring", "abc"])
def test_block_structure_equals_the_reference(dev, gset, hops, chunk, monkeypatch):
    """nodes, level, seed_pos and every block graph's rowptr / colidx / values, for the four seed sets; device and
    host seeds, int32 and int64; a second call is bit-equal.  chunk100: rows of 129 and more entries (and the
    degree-N row) go through the chunk kernels; chunk1024: the rows of 1025 and N entries only."""
    if chunk is not None:
        monkeypatch.setattr(minibatch, "CHUNK", chunk)
    graphs = [_to_gpu(_graph_abc()[i], dev) for i in GRAPH_SETS[gset]]
    for k, (sset, seeds) in enumerate(_seed_sets().items()):
        want = _reference(gset, sset, hops)
        if gset == "ring":
            assert want["nodes"].size == min(N, seeds.size * (hops + 1)) or sset == "some"
        given = (seeds, torch.as_tensor(seeds).to(dev), torch.as_tensor(seeds).to(dev, torch.int32))[(k + hops) % 3]
        blk = minibatch.ego_block(graphs, given, hops)
        _assert_block_equals(blk, want)
        assert blk.n == N
        assert _bit_equal(blk, minibatch.ego_block(graphs, given, hops)), sset
    if chunk is not None and gset == "abc":
        assert graphs[0].row_split(chunk, chunk)["n_long"] >= 5          # the chunk kernels did run


def test_ring_block_sizes(dev):
    """On the directed ring i -> i, i + 1 each hop adds exactly one node per (well separated) seed."""
    g = _to_gpu(_graph_abc()[2], dev)
    seeds = (10, 500, N - 1)
    for hops in (1, 2, 3):
        blk = minibatch.ego_block([g], list(seeds), hops)
        want = {(s + k) % N: k for s in seeds for k in range(hops + 1)}
        assert blk.nodes.numel() == 3 * (hops + 1)
        assert blk.nodes.cpu().tolist() == sorted(want)
        assert blk.level.cpu().tolist() == [want[v] for v in sorted(want)]
        assert [g.nnz for g in blk.graphs] == [3 * (2 * hops + 1)]          # kept rows hold 2 entries, rim rows 1


def test_device_seed_errors(dev):
    g = _to_gpu(_graph_abc()[2], dev)
    with pytest.raises(ValueError, match="repeated"):
        minibatch.ego_block([g], torch.tensor([3, 4, 3], device=dev))
    with pytest.raises(ValueError, match="outside"):
        minibatch.ego_block([g], torch.tensor([3, N], device=dev))
    with pytest.raises(ValueError, match="GPU"):
        minibatch.ego_block([g], torch.tensor([3, 4]))
    with pytest.raises(ValueError, match="GPU"):
        minibatch.ego_block([g, g.to("cpu")], [3])


@pytest.mark.parametrize("binary", [True, False])
def test_sparse_features_take(dev, binary):
    rng = np.random.default_rng(11)
    dense = (rng.random((203, 37)) < 0.08) * (1.0 if binary else rng.standard_normal((203, 37)))
    dense[17] = 0.0                                                  # an empty row
    dense[18] = 1.0 if binary else rng.standard_normal(37)           # a full one
    x = SparseFeatures.from_dense(torch.tensor(dense, dtype=torch.float32, device=dev))
    if binary:
        x = SparseFeatures(x.rowptr, x.colidx, None, x.n_cols)
    full = x.to_dense()
    for ids in (rng.integers(0, 203, 500), np.array([18, 17, 17, 202, 0, 18]), np.array([17]), np.zeros(0, np.int64),
                torch.as_tensor(rng.permutation(203)).to(dev)):
        t = x.take(ids)
        assert (t.values is None) == binary and t.shape == (len(ids), 37)
        assert t.rowptr.dtype == torch.int64 and t.colidx.dtype == torch.int32 and int(t.rowptr[-1]) == t.nnz
        assert torch.equal(t.to_dense(), full[torch.as_tensor(ids).to(dev).long()])
        again = x.take(ids)
        assert torch.equal(t.rowptr, again.rowptr) and torch.equal(t.colidx, again.colidx)
    with pytest.raises(ValueError, match="outside"):
        x.take([0, 203])


# ---- 2. / 3. forward and gradient parity -------------------------------------------------------------------------------
MODELS = {"one_layer": dict(), "two_layers_residual": dict(hid_units=[8, 16], n_heads=(8, 4, 1), residual=True)}


@functools.lru_cache(maxsize=None)
def _problem(name):
    """helpers.make_problem at n = 300 (isolated node 1, hub 2), the float64 oracle outputs on the full graph, and
    the 40 seeds; computed once, read only."""
    kw = MODELS[name]
    prob = make_problem(31, 300, 24, 2, 3, (0.02, 0.1), **kw)
    hid, heads = kw.get("hid_units", [8]), list(kw.get("n_heads", (8, 1)))
    out = ho.hetegat_multi_inference([prob["x"]] * 2, 3, 300, False, 0.0, 0.0, prob["biases"], hid, heads,
                                     prob["params"], residual=kw.get("residual", False))
    rng = np.random.default_rng(5)
    seeds = rng.permutation(np.concatenate([[0, 1], 3 + rng.permutation(297)[:38]]))
    return prob, tuple(np.asarray(o) for o in out), seeds


def _infer(model, name, x, graphs):
    """model.inference as the reference calls it: (logits (N, C), final_embed, att_val)."""
    kw = MODELS[name]
    with torch.no_grad():
        lg, fe, att = model.inference([x] * 2, 3, graphs[0].n_rows, False, 0.0, 0.0, graphs, kw.get("hid_units", [8]),
                                      list(kw.get("n_heads", (8, 1))), residual=kw.get("residual", False))
    return lg[0], fe, att


def _close(got, want, tol, what):
    err = float(np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64)).max())
    print(f"{what}: max abs difference {err:.3e} (bound {tol:g})")
    assert err < tol, (what, err)


@pytest.mark.parametrize("name", list(MODELS))
def test_block_forward_matches_the_full_graph(dev, name):
    """Rows seed_pos of logits / final_embed / att_val on the block against rows `seeds` of the float64 oracle on
    the full graph (1e-4, the bound of test_inference_matches_oracle and of the multi-layer test's forward), and
    against full-graph GPU inference (2e-4: each side is within 1e-4 of the oracle).  The same block fed
    SparseFeatures: the taken rows are the dense rows bit for bit, the outputs within the same bounds (the sparse
    projection adds in another order than the dense one)."""
    prob, oracle, seeds = _problem(name)
    model, _ = build_model(prob, dev)
    x, graphs = gpu_inputs(prob, dev)
    hops = 1 + len(model.extra)
    assert hops == (1 if name == "one_layer" else 2)
    blk = minibatch.ego_block(graphs, seeds, hops)
    print(f"{name}: block of {blk.nodes.numel()} nodes, {int((blk.level == hops).sum())} on the rim, "
          f"nnz {[g.nnz for g in blk.graphs]} of {[g.nnz for g in graphs]}")
    xb = blk.take(x)
    sp = blk.seed_pos
    got = tuple(t[sp] for t in _infer(model, name, xb, blk.graphs))
    full = _infer(model, name, x, graphs)
    for g, o, f, what in zip(got, oracle, full, ("logits", "final_embed", "att_val")):
        o = o[0] if o.ndim == 3 else o
        _close(g.cpu().numpy(), o[seeds], TOL, f"{name} block {what} vs oracle")
        _close(g.cpu().numpy(), f[torch.as_tensor(seeds).to(dev)].cpu().numpy(), 2 * TOL, f"{name} block {what} vs full GPU")
    xs = SparseFeatures.from_dense(x)
    xsb = blk.take(xs)
    assert isinstance(xsb, SparseFeatures) and torch.equal(xsb.to_dense(), xb)
    got2 = tuple(t[sp] for t in _infer(model, name, xsb, blk.graphs))
    for g, g2, o, what in zip(got, got2, oracle, ("logits", "final_embed", "att_val")):
        o = o[0] if o.ndim == 3 else o
        _close(g2.cpu().numpy(), o[seeds], TOL, f"{name} sparse block {what} vs oracle")
        _close(g2.cpu().numpy(), g.cpu().numpy(), 2 * TOL, f"{name} sparse block {what} vs dense block")


@pytest.mark.parametrize("name", list(MODELS))
def test_predict_matches_full_inference(dev, name):
    """predict over all rows in batches of 64 (and over a repeated, unsorted row list) against the oracle and
    full-graph GPU inference."""
    prob, oracle, seeds = _problem(name)
    model, _ = build_model(prob, dev)
    x, graphs = gpu_inputs(prob, dev)
    full = _infer(model, name, x, graphs)
    got = minibatch.predict(model, [x] * 2, graphs, batch_size=64)
    rows = np.concatenate([seeds, seeds[:5], [299, 0]])
    some = minibatch.predict(model, [x[None]] * 2, graphs, rows=rows, batch_size=16)
    for g, s, o, f, what in zip(got, some, oracle, full, ("logits", "final_embed", "att_val")):
        o = o[0] if o.ndim == 3 else o
        assert g.shape == f.shape and s.shape == (rows.size,) + tuple(f.shape[1:])
        _close(g.cpu().numpy(), o, TOL, f"{name} predict {what} vs oracle")
        _close(g.cpu().numpy(), f.cpu().numpy(), 2 * TOL, f"{name} predict {what} vs full GPU")
        _close(s.cpu().numpy(), o[rows], TOL, f"{name} predict(rows) {what} vs oracle")


@pytest.mark.parametrize("name", list(MODELS))
def test_block_gradient_matches_the_full_graph_oracle(dev, name):
    """Dropout 0, loss over the seeds only: model.flat_grad from the block against float64 autograd of the full-graph
    loss masked to the seeds (2e-3 relative to the largest element, per parameter, as the suite's gradient tests)."""
    prob, _, seeds = _problem(name)
    model, bp = build_model(prob, dev)
    x, graphs = gpu_inputs(prob, dev)
    mask = np.zeros(300, dtype=bool)
    mask[seeds] = True
    bpo = {k: v.clone().requires_grad_(True) for k, v in bp.items()}
    og = [tuple(torch.tensor(t) for t in ho.bias_to_csr(b)) for b in prob["biases"]]
    lg_ref, _, _ = ht.hetegat_forward([torch.tensor(prob["x"][0])] * 2, og, bpo, keep_in=1.0, keep_coef=1.0)
    loss_ref = ht.masked_softmax_cross_entropy(lg_ref, torch.tensor(prob["onehot"]), torch.tensor(mask))
    loss_ref.backward()

    blk = minibatch.ego_block(graphs, seeds, 1 + len(model.extra))
    labels = blk.take(torch.tensor(prob["labels"], dtype=torch.int32, device=dev))
    bmask = torch.zeros(blk.nodes.numel(), dtype=torch.uint8, device=dev)
    bmask[blk.seed_pos] = 1
    model.zero_grad_flat()
    M = model.node_level([blk.take(x)] * 2, blk.graphs, 0.0, 0.0, True, ops.ACT_ELU)
    Z, _ = model.semantic(M)
    loss, _, _ = model.classifier_loss(Z, labels, bmask, 1.0 / seeds.size)
    loss.backward()
    print(f"{name}: loss {float(loss.detach()):.6f} vs oracle {float(loss_ref.detach()):.6f}")
    assert abs(float(loss.detach()) - float(loss_ref.detach())) < 5e-4 * max(1.0, float(loss_ref.detach()))
    assert sorted(k for k, _ in model.param_shapes()) == sorted(ht.param_order(bp))
    for k, _ in model.param_shapes():                   # the layout of model.flat_grad
        err = rel_err(getattr(model, k).grad.cpu().numpy(), bpo[k].grad.numpy())
        print(f"{name}: grad {k} rel err {err:.3e}")
        assert err < GTOL, k
    want = np.concatenate([bpo[k].grad.numpy().ravel() for k, _ in model.param_shapes()])
    assert model.flat_grad.shape == want.shape


# ---- 4. trainer parity ---------------------------------------------------------------------------------------------------
def test_one_batch_of_all_training_nodes_is_the_full_graph_trainer(dev):
    """Dropout 0, one batch = all training nodes: three MiniBatchTrainer steps against three HANTrainer.train_steps,
    parameters within 2e-4 (the suite's three-step bound)."""
    from han_amd.trainer import HANTrainer
    prob = make_problem(11, 80, 16, 2, 3, [0.05, 0.4])
    x, graphs = gpu_inputs(prob, dev)
    labels = torch.tensor(prob["labels"], dtype=torch.int32, device=dev)
    tm = torch.tensor(prob["mask"].astype(np.uint8))
    full_model, _ = build_model(prob, dev)
    mini_model, _ = build_model(prob, dev)
    full = HANTrainer(full_model, [x] * 2, graphs, labels, tm, lr=0.005, l2_coef=0.001, attn_drop=0.0, ffd_drop=0.0)
    mini = minibatch.MiniBatchTrainer(mini_model, [x] * 2, graphs, labels, tm, batch_size=80, lr=0.005, l2_coef=0.001,
                                      attn_drop=0.0, ffd_drop=0.0, seed=1)
    assert len(mini.batches()) == 1 and mini.batches()[0].size == int(prob["mask"].sum())
    for _ in range(3):
        fl, fa = full.train_step()
        (b,) = mini.batches()
        ml, ma = mini.train_step(b)
        mini.epochs_done += 1
        assert abs(float(fl) - float(ml)) < 2e-4 and abs(float(fa) - float(ma)) < 1e-5
    for k in ht.PARAM_ORDER:
        err = float((getattr(full_model, k) - getattr(mini_model, k)).detach().abs().max())
        print(f"param {k}: max abs difference {err:.3e}")
        assert err < 2e-4, k
    vl, va = mini.evaluate(tm)                          # the same parameters through predict and through eval_step
    same = HANTrainer(mini_model, [x] * 2, graphs, labels, tm, attn_drop=0.0, ffd_drop=0.0)
    fl, fa = same.eval_step(same.train_mask, same.w_train)
    assert abs(float(vl) - float(fl)) < 2e-4 and abs(float(va) - float(fa)) < 1e-5


def test_equal_seeds_give_bit_equal_runs(dev):
    prob = make_problem(11, 80, 16, 2, 3, [0.05, 0.4])
    x, graphs = gpu_inputs(prob, dev)
    labels = torch.tensor(prob["labels"], dtype=torch.int32, device=dev)
    tm = torch.tensor(prob["mask"].astype(np.uint8))

    def run(seed):
        model, _ = build_model(prob, dev)
        tr = minibatch.MiniBatchTrainer(model, [x] * 2, graphs, labels, tm, batch_size=12, attn_drop=0.6,
                                        ffd_drop=0.6, seed=seed)
        for _ in range(2):
            tr.epoch()
        return model.flat.detach().clone()

    a, b, c = run(4), run(4), run(5)
    assert torch.isfinite(a).all() and torch.equal(a, b)
    assert not torch.equal(a, c)


# ---- 5. learning ---------------------------------------------------------------------------------------------------------
def test_minibatch_training_learns_planted_communities(dev):
    """The workload and the bar of test_training_learns_planted_communities (chance 0.25), in batches of 100 seeds with
    dropout 0.6 / 0.6, at most 100 epochs with early stopping."""
    from han_amd import synth
    from han_amd.gat import HeteGAT_multi
    torch.manual_seed(0)
    wl = synth.planted_partition(1500, 4, 2, 32, deg_in=8, deg_out=2, noise=1.0, seed=3, device=dev)
    model = HeteGAT_multi().build(2, 32, 4, (8,), (8, 1), 128, device=dev)
    tr = minibatch.MiniBatchTrainer(model, [wl["x"]] * 2, wl["graphs"], wl["labels"], wl["train_mask"], wl["val_mask"],
                                    batch_size=100, attn_drop=0.6, ffd_drop=0.6, seed=5, patience=30)
    for epoch in range(100):
        tl, ta, vl, va = (float(v) for v in tr.epoch())
        if tr.early_stopping(vl, va):
            break
    tr.restore_best()
    loss, acc = tr.evaluate(wl["test_mask"])
    print(f"{epoch + 1} epochs, test loss {float(loss):.4f}, test accuracy {float(acc):.4f}")
    assert float(acc) > 0.9, float(acc)
