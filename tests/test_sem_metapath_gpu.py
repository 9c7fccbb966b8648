"""GPU tests of han_amd/csrc/sem_attn_mean.hip (K3 as published, han.pdf eq. 7-9: one weight per meta-path) through the
C ABI (han_sem_attn_mean_fwd / _bwd via han_amd.ops) and of semantic="metapath" at model level.

Tolerances are the project's: Z, beta and w within 1e-4 absolute of the float64 reference
(tests/sem_metapath_ref.py), gradients within 2e-3 of the largest magnitude of the tensor or of the sub-tensor named in
the test.  Every comparison prints its figure before it asserts."""
import functools

import numpy as np
import pytest
import torch

from oracle import han_oracle_torch as ht
from tests import sem_metapath_cpu, sem_metapath_ref as ref
from tests.helpers import gpu_inputs, load_params, make_problem

pytestmark = pytest.mark.gpu

ATOL = 1e-4      # Z, beta, w: absolute
GTOL = 2e-3      # gradients: of the largest magnitude of the (sub-)tensor

SHAPES = [(1, 2, 64, 64), (5, 3, 64, 128), (67, 1, 64, 64), (67, 5, 64, 128), (1000, 4, 64, 128), (333, 8, 128, 256),
          (129, 3, 64, 192), (50, 64, 64, 64)]


def _u_scale(i):
    return 10.0 if i % 2 else 1.0      # half of the shapes with beta far from uniform


def _gpu(dev, *xs):
    return tuple(torch.tensor(np.ascontiguousarray(x), device=dev) for x in xs)


def _run(dev, inp):
    """Forward and backward of the GPU kernels on fp32 NumPy inputs (M, W, b, u, dZ); NumPy results and the GPU beta."""
    from han_amd import ops
    M, W, b, u, dZ = _gpu(dev, *inp)
    Z, beta, w = ops.sem_attn_mean_fwd(M, W, b, u, want_mean=True)
    dM, dw, db, du = ops.sem_attn_mean_bwd(M, W, b, u, beta, dZ)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in dict(Z=Z, beta=beta, w=w, dM=dM, dw=dw, db=db, du=du).items()}


def _abs_close(got, want, name):
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(f"{name}: max abs err {err:.3e} (bound {ATOL:.0e})")
    assert err <= ATOL, name


def _grad_close(got, want, name):
    err, top = float(np.abs(got.astype(np.float64) - want).max()), float(np.abs(want).max())
    print(f"{name}: max abs err {err:.3e}, largest magnitude {top:.3e}, ratio {err / max(top, 1e-300):.3e} (bound {GTOL:.0e})")
    assert err <= GTOL * top, name      # an all-zero gradient (P = 1) has to be matched exactly


def _check_all(got, inp, tag):
    M, W, b, u, dZ = inp
    Z, beta, w = ref.forward(M, W, b, u)
    _abs_close(got["Z"], Z, tag + " Z")
    _abs_close(got["beta"], beta, tag + " beta")
    _abs_close(got["w"], w, tag + " w")
    for name, want in zip(("dM", "dw", "db", "du"), ref.backward(M, W, b, u, dZ)):
        _grad_close(got[name], want, f"{tag} {name}")
    return beta


# --------------------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("i", range(len(SHAPES)), ids=["x".join(map(str, s)) for s in SHAPES])
def test_forward_and_backward_parity(dev, i):
    N, P, D, A = SHAPES[i]
    inp = ref.inputs(N, P, D, A, seed=100 + i, u_scale=_u_scale(i))
    got = _run(dev, inp)
    beta = _check_all(got, inp, f"{SHAPES[i]}")
    if P > 1 and _u_scale(i) > 1 and N <= 67:
        assert beta.max() > 1.2 / P      # the scaled u did move beta away from uniform
    assert abs(float(got["beta"].sum()) - 1.0) < 1e-5


# --------------------------------------------------------------------------- 2. the coupling term on its own
@pytest.mark.parametrize("shape", [(1000, 4, 64, 128), (67, 5, 64, 128)], ids=lambda s: "x".join(map(str, s)))
def test_coupling_term_on_rows_without_dz(dev, shape):
    """dZ is non-zero only in the first 7 nodes: on every other row dM_ip = W dpre_ip alone, N times smaller than the
    direct term, and compared relative to the largest magnitude AMONG THOSE ROWS."""
    N, P, D, A = shape
    M, W, b, u, dZ = ref.inputs(N, P, D, A, seed=7 * N, u_scale=10.0)
    dZ[7:] = 0.0
    got = _run(dev, (M, W, b, u, dZ))
    dM = ref.backward(M, W, b, u, dZ)[0]
    assert 0 < np.abs(dM[7:]).max() < np.abs(dM[:7]).max()
    _grad_close(got["dM"][7:], dM[7:], f"{shape} dM, rows without dZ")
    _grad_close(got["dM"][:7], dM[:7], f"{shape} dM, rows of the first 7 nodes")


# --------------------------------------------------------------------------- 3. P = 1
def test_single_metapath_is_the_identity(dev):
    inp = ref.inputs(67, 1, 64, 64, seed=3, u_scale=10.0)
    got = _run(dev, inp)
    assert got["beta"].tolist() == [1.0]
    assert np.array_equal(got["Z"], inp[0][:, 0]) and np.array_equal(got["dM"][:, 0], inp[4])
    for k in ("dw", "db", "du"):
        assert not got[k].any(), k


# --------------------------------------------------------------------------- 4. against the existing kernels
@pytest.mark.parametrize("N, tiled", [(200, True), (1, False)])
def test_against_the_per_node_kernels(dev, N, tiled):
    """Where every node carries the same (P, D) block -- or there is one node -- the per-node softmax and the softmax of
    the node means coincide: han_sem_attn_fwd / han_sem_attn_bwd are an independent reference."""
    from han_amd import ops
    P, D, A = 4, 64, 128
    M, W, b, u, dZ = ref.inputs(N, P, D, A, seed=41 + N, u_scale=10.0)
    if tiled:
        M = np.tile(M[:1], (N, 1, 1))
    got = _run(dev, (M, W, b, u, dZ))
    Mg, Wg, bg, ug, dZg = _gpu(dev, M, W, b, u, dZ)
    Zn, betan = ops.sem_attn_fwd(Mg, Wg, bg, ug)
    dMn, dwn, dbn, dun = ops.sem_attn_bwd(Mg, Wg, bg, ug, betan, dZg)
    f64 = lambda t: t.cpu().numpy().astype(np.float64)
    _abs_close(got["Z"], f64(Zn), "Z")
    _abs_close(np.broadcast_to(got["beta"], (N, P)), f64(betan), "beta, every row")
    _grad_close(got["dw"], f64(dwn), "dw")
    _grad_close(got["db"], f64(dbn), "db")
    _grad_close(got["du"], f64(dun), "du")
    _grad_close(got["dM"].astype(np.float64).sum(0), f64(dMn).sum(0), "sum_i dM_i")


# --------------------------------------------------------------------------- 5. every block loops
def _loop_shape():
    from han_amd import ops
    rows = 2 * ops.SEM_MEAN_GRID_CAP * ops.SEM_MEAN_ROWS_PER_BLOCK + 37
    return (-(-rows // 3), 3, 64, 64)


@functools.lru_cache(maxsize=None)
def _loop_case():
    """Inputs and float64 reference of the case in which every block of every kernel runs its loop at least twice and the
    slabs have their full height; computed once, shared, and not modified."""
    N, P, D, A = _loop_shape()
    inp = ref.inputs(N, P, D, A, seed=5, u_scale=10.0)
    return inp, ref.forward(*inp[:4]), ref.backward(*inp)


def test_every_block_loops(dev):
    from han_amd import ops
    N, P, D, A = _loop_shape()
    cap, rows = ops.SEM_MEAN_GRID_CAP, ops.SEM_MEAN_ROWS_PER_BLOCK
    assert N * P >= 2 * cap * rows + 37
    assert N * (D // 4) >= 2 * cap * 256      # the combine kernel: 256 threads x 4 features per block iteration
    inp, (Z, beta, w), (dM, dw, db, du) = _loop_case()
    got = _run(dev, inp)
    _abs_close(got["beta"], beta, "beta")
    _abs_close(got["w"], w, "w")
    _grad_close(got["dw"], dw, "dw")
    _grad_close(got["db"], db, "db")
    _grad_close(got["du"], du, "du")
    # the first and the last node, nodes that straddle a boundary between two blocks' 64-row ranges (also the wrap from
    # the last block of a grid pass to the first), and random ones
    straddle = [(rows * k) // P for k in (1, 2, 5, cap - 1, cap, cap + 1, 2 * cap - 1, 2 * cap) if (rows * k) % P]
    assert len(straddle) >= 4 and all((n * P) // rows != (n * P + P - 1) // rows for n in straddle)
    fixed = sorted({0, N - 1, *straddle})
    pool = [int(n) for n in np.random.default_rng(0).permutation(N)[:80] if n not in fixed]
    nodes = np.array(sorted(fixed + pool[:64 - len(fixed)]))
    assert len(nodes) == 64 and nodes.max() == N - 1
    _abs_close(got["Z"][nodes], Z[nodes], "Z, sampled nodes")
    _grad_close(got["dM"][nodes], dM[nodes], "dM, sampled nodes")


# --------------------------------------------------------------------------- 6. determinism
@pytest.mark.parametrize("which", ["loop", "67x5x64x128"])
def test_results_are_bit_identical_from_run_to_run(dev, which):
    inp = _loop_case()[0] if which == "loop" else ref.inputs(67, 5, 64, 128, seed=9, u_scale=10.0)
    a, b = _run(dev, inp), _run(dev, inp)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


# --------------------------------------------------------------------------- 7. return codes
def test_return_codes(dev):
    from han_amd import _lib
    lib = _lib.load()
    E_WORKSPACE = -3

    def call(N, P, D, A, short=0):
        t = lambda *s: torch.full(s, 7.0, device=dev)
        M, W, b, u, dZ = t(max(N, 1), P, D), t(D, A), t(A), t(A), t(max(N, 1), D)
        Z, beta, dM, dw, db, du = t(max(N, 1), D), t(P), t(max(N, 1), P, D), t(D, A), t(A), t(A)
        need = lib.han_sem_attn_mean_workspace(N, P, D, A)
        ws = torch.zeros(max(need, 1), dtype=torch.uint8, device=dev)
        f = lib.han_sem_attn_mean_fwd(M.data_ptr(), W.data_ptr(), b.data_ptr(), u.data_ptr(), Z.data_ptr(), beta.data_ptr(),
                                      None, ws.data_ptr(), need - short, N, P, D, A, 0, None)
        g = lib.han_sem_attn_mean_bwd(M.data_ptr(), W.data_ptr(), b.data_ptr(), u.data_ptr(), beta.data_ptr(), dZ.data_ptr(),
                                      dM.data_ptr(), dw.data_ptr(), db.data_ptr(), du.data_ptr(), ws.data_ptr(),
                                      need - short, N, P, D, A, 0, None)
        torch.cuda.synchronize()
        untouched = all(bool((x == 7).all()) for x in (Z, beta, dM, dw, db, du))
        return f, g, untouched

    assert call(10, 3, 192, 64) == (_lib.E_UNSUPPORTED, _lib.E_UNSUPPORTED, True)
    assert call(10, 3, 64, 320) == (_lib.E_UNSUPPORTED, _lib.E_UNSUPPORTED, True)
    assert call(10, 65, 64, 64) == (_lib.E_UNSUPPORTED, _lib.E_UNSUPPORTED, True)
    assert call(10, 3, 64, 128, short=1) == (E_WORKSPACE, E_WORKSPACE, True)
    assert call(0, 3, 64, 128) == (0, 0, True)
    f, g, untouched = call(10, 3, 64, 128)
    assert (f, g) == (0, 0) and not untouched


# --------------------------------------------------------------------------- 8. model level
N_MODEL = 257


def _model_problem():
    return make_problem(88, N_MODEL, 40, 3, 3, [0.05, 0.3, 0.1])


def _build(prob, dev, semantic):
    from han_amd.gat import HeteGAT_multi
    model = HeteGAT_multi().build(prob["p"], prob["f"], prob["c"], (8,), (8, 1), 128, device=dev, semantic=semantic)
    bp = ht.to_batched(prob["params"])
    load_params(model, bp)
    return model, bp


def _trainer(prob, dev, model, **kw):
    from han_amd.trainer import HANTrainer
    x, graphs = gpu_inputs(prob, dev)
    t = lambda a, dt: torch.tensor(a, dtype=dt, device=dev)
    return HANTrainer(model, [x] * prob["p"], graphs, t(prob["labels"], torch.int32),
                      t(prob["mask"].astype(np.uint8), torch.uint8), t((~prob["mask"]).astype(np.uint8), torch.uint8), **kw)


def test_model_forward_loss_and_gradients_match_the_oracle(dev):
    prob = _model_problem()
    model, bp = _build(prob, dev, "metapath")
    tr = _trainer(prob, dev, model, attn_drop=0.0, ffd_drop=0.0)
    assert not tr.live_forward and not tr.live_backward
    loss_ref, logits_ref, embed_ref, beta_ref, grads = sem_metapath_cpu.loss_and_grads(prob, bp)
    model.zero_grad_flat()
    loss, _ = tr._forward(True, tr.train_mask, tr.w_train)
    loss.backward()
    torch.cuda.synchronize()
    print(f"loss {float(loss.detach()):.6f} vs {loss_ref:.6f}")
    assert abs(float(loss.detach()) - loss_ref) <= ATOL
    for k in ht.PARAM_ORDER:
        _grad_close(getattr(model, k).grad.cpu().numpy(), grads[k], f"d {k}")
    x, graphs = gpu_inputs(prob, dev)
    with torch.no_grad():
        logits, embed, att = model.inference([x] * 3, 3, N_MODEL, False, 0.0, 0.0, graphs, [8], [8, 1],
                                             semantic="metapath")
    _abs_close(logits[0].cpu().numpy(), logits_ref, "logits")
    _abs_close(embed.cpu().numpy(), embed_ref, "final_embed")
    assert att.shape == (N_MODEL, 3) and att.stride(0) == 0
    att = att.cpu().numpy()
    assert (att == att[0]).all() and abs(float(att[0].astype(np.float64).sum()) - 1.0) < 1e-5
    _abs_close(att[0], beta_ref, "att_val row")
    # fold_k3, which the trainer sets, has no effect in this mode: no FoldTail is produced.  The node mode of the same
    # variables produces one, and gives other numbers: the keyword does select the arithmetic
    from han_amd import ops
    node, _ = _build(prob, dev, "node")
    trn = _trainer(prob, dev, node, attn_drop=0.0, ffd_drop=0.0)
    for t, folds in ((tr, False), (trn, True)):
        assert t.model.fold_k3
        t.model.node_level(t.xs, t.graphs, 0.0, 0.0, True, ops.ACT_ELU, graphs_t=t.graphs_t)
        assert (t.model._fold_handover is not None) == folds
        t.model._fold_handover = None
    with torch.no_grad():
        embed_n = node.inference([x] * 3, 3, N_MODEL, False, 0.0, 0.0, graphs, [8], [8, 1])[1]
    assert float((embed_n - embed).abs().max()) > 1e-3


def test_three_trainer_steps_eager_and_captured_agree(dev):
    """As test_gpu_parity.test_captured_epoch_replay_matches_eager_and_oracle: the captured epoch against the identical
    device-state flow launched eagerly -- the same losses, bitwise the same parameters."""
    from han_amd import rng as hrng
    prob = _model_problem()
    trainers = []
    for capture in (True, False):
        model, _ = _build(prob, dev, "metapath")
        tr = _trainer(prob, dev, model, attn_drop=0.6, ffd_drop=0.6, use_graph=True)
        tr._capture = capture
        trainers.append(tr)
    for ep in range(3):
        outs = []
        for tr in trainers:
            if ep == 0:
                hrng.manual_seed(77)
            outs.append([float(v) for v in tr.epoch()])
        assert outs[0] == outs[1] and all(np.isfinite(outs[0])), (ep, outs)
    assert trainers[0]._graph is not None and trainers[1]._graph is None
    assert torch.equal(trainers[0].model.flat, trainers[1].model.flat)


def test_live_forward_raises(dev):
    prob = _model_problem()
    model, _ = _build(prob, dev, "metapath")
    with pytest.raises(ValueError, match="metapath"):
        _trainer(prob, dev, model, live_forward=True)
    with pytest.raises(ValueError, match="metapath"):
        _trainer(prob, dev, model, live_backward=True)
