"""Host tests (no GPU) of semantic="metapath" (han.pdf eq. 7-9, one weight per meta-path): the closed-form backward of
tests/sem_metapath_ref.py against float64 autograd, and the wiring above the C ABI -- default mode, what must decline
in the new mode, the mode in state_dict / checkpoints -- with the kernels replaced by tests/sem_metapath_cpu.py."""
import numpy as np
import pytest
import torch

from oracle import han_oracle_torch as ht
from tests import sem_metapath_cpu, sem_metapath_ref as ref
from tests.helpers import load_params, make_problem, rel_err


@pytest.fixture()
def cpu_ops(monkeypatch):
    return sem_metapath_cpu.install(monkeypatch)


def _graphs(prob):
    from han_amd.graph import CSRGraph
    return [CSRGraph.from_bias(torch.tensor(b, dtype=torch.float32)) for b in prob["biases"]]


def _model(prob, semantic):
    from han_amd.gat import HeteGAT_multi
    model = HeteGAT_multi().build(prob["p"], prob["f"], prob["c"], device="cpu", semantic=semantic)
    bp = ht.to_batched(prob["params"])
    load_params(model, bp)
    return model, bp


def _trainer(prob, semantic="metapath", **kw):
    from han_amd.trainer import HANTrainer
    model, bp = _model(prob, semantic)
    x = torch.tensor(prob["x"][0], dtype=torch.float32)
    tr = HANTrainer(model, [x] * prob["p"], _graphs(prob), torch.tensor(prob["labels"], dtype=torch.int32),
                    torch.tensor(prob["mask"].astype(np.uint8)), attn_drop=0.0, ffd_drop=0.0, **kw)
    return tr, bp


# --------------------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("shape", [(5, 3, 64, 64), (37, 4, 128, 192)])
def test_closed_form_backward_matches_float64_autograd(shape):
    N, P, D, A = shape
    M, W, b, u, dZ = ref.up(*ref.inputs(N, P, D, A, seed=N + P, u_scale=10.0))
    t = [torch.tensor(x, requires_grad=True) for x in (M, W, b, u)]
    v = torch.tanh(t[0] @ t[1] + t[2])
    w = (v @ t[3]).mean(0)
    beta = torch.softmax(w, dim=0)
    Z = (beta[None, :, None] * t[0]).sum(1)
    (Z * torch.tensor(dZ)).sum().backward()
    Zr, betar, wr = ref.forward(M, W, b, u)
    assert rel_err(Zr, Z.detach().numpy()) < 1e-12 and rel_err(betar, beta.detach().numpy()) < 1e-12
    assert rel_err(wr, w.detach().numpy()) < 1e-12
    assert betar.max() > 1.5 / P      # far from uniform: the softmax Jacobian takes part
    for got, want, name in zip(ref.backward(M, W, b, u, dZ), t, ("dM", "dW", "db", "du")):
        assert rel_err(got, want.grad.numpy()) < 1e-10, name


def test_the_two_modes_differ_and_coincide_where_they_must():
    """Different results on random rows (the test would otherwise show nothing); the same where every node carries the
    same (P, D) block."""
    M, W, b, u, _ = ref.inputs(40, 3, 64, 64, seed=1, u_scale=10.0)
    node = ht.semantic_attention(*(torch.tensor(x, dtype=torch.float64) for x in (M, W, b, u)))[0].numpy()
    assert np.abs(ref.forward(M, W, b, u)[0] - node).max() > 1e-2
    Mt = np.tile(M[:1], (40, 1, 1))
    node = ht.semantic_attention(*(torch.tensor(x, dtype=torch.float64) for x in (Mt, W, b, u)))
    Z, beta, _ = ref.forward(Mt, W, b, u)
    assert np.abs(Z - node[0].numpy()).max() < 1e-12 and np.abs(beta - node[1].numpy()[7]).max() < 1e-12


# --------------------------------------------------------------------------- wiring
def test_default_mode_is_node():
    import inspect
    from han_amd import layers
    from han_amd.gat import HeteGAT, HeteGAT_multi, HeteGAT_no_coef
    assert HeteGAT_multi().semantic_mode == "node"
    assert HeteGAT_multi().build(2, 5, 3, device="cpu").semantic_mode == "node"
    for fn in (HeteGAT_multi.build, layers.semantic_attention, layers.SimpleAttLayer):
        par = inspect.signature(fn).parameters
        assert par["semantic" if "semantic" in par else "mode"].default == "node", fn
    for cls in (HeteGAT_multi, HeteGAT, HeteGAT_no_coef):
        par = inspect.signature(cls.__dict__["inference"].fn).parameters
        assert list(par)[-1] == "semantic" and par["semantic"].default == "node"
    with pytest.raises(ValueError, match="semantic"):
        HeteGAT_multi().build(2, 5, 3, device="cpu", semantic="paper")


def test_model_gradients_match_the_oracle_on_cpu_backend(cpu_ops):
    """node_level -> SemanticAttentionMean -> classifier: autograd wiring and direct gradients against float64 autograd
    of the oracle composed with the reference; att_val is beta on every row."""
    prob = make_problem(23, 45, 9, 3, 3, [0.1, 0.4, 0.2])
    tr, bp = _trainer(prob)
    assert tr.model.fold_k3 and not tr.live_forward and not tr.live_backward
    tr.model.zero_grad_flat()
    loss, _ = tr._forward(True, tr.train_mask, tr.w_train)
    loss.backward()
    loss_ref, logits_ref, _, beta_ref, grads = sem_metapath_cpu.loss_and_grads(prob, bp)
    assert abs(float(loss.detach()) - loss_ref) < 1e-5
    for k in ht.PARAM_ORDER:
        assert rel_err(getattr(tr.model, k).grad.numpy(), grads[k]) < 1e-4, k
    with torch.no_grad():      # the stages of inference() (which itself takes GPU tensors only)
        x = torch.tensor(prob["x"][0], dtype=torch.float32)
        Z, att = tr.model.semantic(tr.model.node_level([x] * 3, _graphs(prob), 0.0, 0.0, False, 1))
        logits = tr.model.classify(Z)
    assert np.abs(logits.numpy() - logits_ref).max() < 1e-4
    assert att.shape == (45, 3) and att.stride(0) == 0
    assert np.abs(att[17].numpy() - beta_ref).max() < 1e-6 and abs(float(att[0].sum()) - 1.0) < 1e-6


def test_simple_att_layer_takes_the_mode(cpu_ops):
    from han_amd import layers
    M, W, b, u, _ = (torch.tensor(x) for x in ref.inputs(9, 2, 64, 64, seed=3))
    params = {"w_omega": W, "b_omega": b, "u_omega": u}
    out, al = layers.SimpleAttLayer(M, 64, return_alphas=True, params=params, semantic="metapath")
    Z, beta, _ = ref.forward(M.numpy(), W.numpy(), b.numpy(), u.numpy())
    assert np.abs(out.numpy() - Z).max() < 1e-6 and np.abs(al.numpy() - beta[None]).max() < 1e-6
    out_n = layers.SimpleAttLayer(M, 64, params=params)
    assert torch.equal(out_n, layers.SimpleAttLayer(M, 64, params=params, semantic="node"))
    assert not torch.allclose(out_n, out)


def test_padding_is_exact_and_unsupported_shapes_name_the_supported_set(cpu_ops):
    from han_amd import layers
    M, W, b, u, _ = (torch.tensor(x) for x in ref.inputs(9, 2, 64, 128, seed=4))
    Z, att = layers.semantic_attention(M[:, :, :40].contiguous(), W[:40, :100].contiguous(), b[:100].contiguous(),
                                       u[:100].contiguous(), mode="metapath")
    Zr, beta, _ = ref.forward(M[:, :, :40].numpy(), W[:40, :100].numpy(), b[:100].numpy(), u[:100].numpy())
    assert Z.shape == (9, 40) and np.abs(Z.numpy() - Zr).max() < 1e-6 and np.abs(att[0].numpy() - beta).max() < 1e-6
    wide = torch.zeros(4, 2, 192)
    with pytest.raises(NotImplementedError, match=r"\(64, 128\).*\(64, 128, 192, 256\)"):
        layers.semantic_attention(wide, torch.zeros(192, 64), torch.zeros(64), torch.zeros(64), mode="metapath")
    with pytest.raises(NotImplementedError, match="256"):
        layers.semantic_attention(M, torch.zeros(64, 320), torch.zeros(320), torch.zeros(320), mode="metapath")
    with pytest.raises(ValueError, match="semantic"):
        layers.semantic_attention(M, W, b, u, mode="mean")


def test_inference_checks_the_mode_against_the_built_model(cpu_ops):
    prob = make_problem(5, 30, 7, 2, 3, [0.2, 0.4])
    model, _ = _model(prob, "metapath")
    x = torch.tensor(prob["x"][0], dtype=torch.float32)
    args = ([x, x], 3, None, None, 0.0, 0.0, _graphs(prob), [8], [8, 1])
    with torch.no_grad():      # (a matching call goes on to ask for GPU tensors: tests/test_sem_metapath_gpu.py)
        with pytest.raises(ValueError, match="does not match the model"):
            model.inference(*args)
        with pytest.raises(ValueError, match="does not match the model"):
            model.inference(*args, semantic="node")
        node, _ = _model(prob, "node")
        with pytest.raises(ValueError, match="does not match the model"):
            node.inference(*args, semantic="metapath")
        with pytest.raises(ValueError, match="expected one of"):
            node.inference(*args, semantic="paper")


def test_what_relies_on_row_locality_declines(cpu_ops):
    prob = make_problem(7, 40, 7, 2, 3, [0.2, 0.4])
    for kw in ({"live_forward": True}, {"live_backward": True}, {"masked_backward": True}):
        with pytest.raises(ValueError, match="metapath"):
            _trainer(prob, **kw)
    tr, _ = _trainer(prob, live_forward="auto", live_backward="auto")
    assert not tr.live_forward and not tr.live_backward and tr.model.live_bwd is None
    with pytest.raises(ValueError, match="metapath"):
        tr.set_masked_backward(True)
    tr.epoch()      # and the plain step runs


def test_node_partition_raises(cpu_ops):
    from han_amd.trainer import HANTrainer

    class Part:      # only what the trainer looks at before it declines
        active = True
    prob = make_problem(8, 30, 7, 2, 3, [0.2, 0.4])
    model, _ = _model(prob, "metapath")
    x = torch.tensor(prob["x"][0], dtype=torch.float32)
    with pytest.raises(NotImplementedError, match="partition"):
        HANTrainer(model, [x, x], _graphs(prob), torch.tensor(prob["labels"], dtype=torch.int32),
                   torch.tensor(prob["mask"].astype(np.uint8)), part=Part())
    model.partition = Part()
    with pytest.raises(NotImplementedError, match="partition"):
        model.node_level([x, x], _graphs(prob), 0.0, 0.0, False, 1)


def test_ego_blocks_raise(cpu_ops):
    from han_amd import minibatch
    prob = make_problem(9, 30, 7, 2, 3, [0.2, 0.4])
    model, _ = _model(prob, "metapath")
    x = torch.tensor(prob["x"][0], dtype=torch.float32)
    with pytest.raises(ValueError, match="metapath"):
        minibatch.predict(model, [x, x], _graphs(prob))
    with pytest.raises(ValueError, match="metapath"):
        minibatch.MiniBatchTrainer(model, [x, x], _graphs(prob), torch.tensor(prob["labels"], dtype=torch.int32),
                                   torch.tensor(prob["mask"].astype(np.uint8)))


def test_the_mode_survives_state_dict_and_mismatches_raise(cpu_ops, tmp_path):
    prob = make_problem(10, 30, 7, 2, 3, [0.2, 0.4])
    mp, _ = _model(prob, "metapath")
    node, _ = _model(prob, "node")
    sd = mp.state_dict()
    assert sd["semantic"] == "metapath" and "semantic" not in node.state_dict()
    assert set(sd) - {"semantic"} == set(node.state_dict())
    other, _ = _model(make_problem(11, 30, 7, 2, 3, [0.2, 0.4]), "metapath")
    other.load_state_dict(sd)
    assert torch.equal(other.flat, mp.flat) and other.semantic_mode == "metapath"
    with pytest.raises(ValueError, match="semantic"):
        node.load_state_dict(sd)
    with pytest.raises(ValueError, match="semantic"):
        mp.load_state_dict(node.state_dict())
    # the trainer's checkpoints
    tr, _ = _trainer(prob)
    tr.epoch()
    path = str(tmp_path / "ck.pt")
    tr.save_checkpoint(path)
    tr2, _ = _trainer(prob)
    tr2.load_checkpoint(path)
    assert torch.equal(tr2.model.flat, tr.model.flat)
    trn, _ = _trainer(prob, semantic="node")
    assert "semantic" not in trn._signature()
    with pytest.raises(ValueError, match="different model"):
        trn.load_checkpoint(path)
    trn.save_checkpoint(path)
    with pytest.raises(ValueError, match="different model"):
        tr2.load_checkpoint(path)
