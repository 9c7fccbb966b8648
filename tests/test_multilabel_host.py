"""Host tests of the multi-label objective: the float64 reference with bounds (tests/multilabel_ref.py) that
tests/test_multilabel_gpu.py holds the kernels to, against BaseGAttN.masked_sigmoid_cross_entropy / micro_f1 and torch
autograd in float64; the label packing; the constructor checks of HANTrainer(objective="sigmoid"); and the
preconditions of the shared seeded inputs (no undecided prediction on a live row, so the GPU file may demand exact
counts)."""
import math

import numpy as np
import pytest
import torch

from han_amd import ops, synth
from han_amd.base_gattn import BaseGAttN
from tests import multilabel_ref as R


def _torch_oracle(case):
    """loss, dlogits, dZ, dWc, dbc by autograd in float64 from the reference's own expressions."""
    Z = torch.tensor(R.up(case["Z"]), requires_grad=True)
    Wc = torch.tensor(R.up(case["Wc"]), requires_grad=True)
    bc = torch.tensor(R.up(case["bc"]), requires_grad=True)
    logits = (Z @ Wc.mean(0) + bc.mean(0))
    logits.retain_grad()
    mask = torch.tensor((case["mask"] != 0).astype(np.float64))
    loss = BaseGAttN.masked_sigmoid_cross_entropy(logits, torch.tensor(case["y"].astype(np.float64)), mask)
    loss.backward()
    return logits.detach(), loss.item(), logits.grad, Z.grad, Wc.grad, bc.grad


@pytest.mark.parametrize("D,C,HC,N", [(64, 3, 1, 65), (128, 33, 2, 63), (320, 17, 3, 17), (64, 100, 1, 15)])
def test_reference_agrees_with_base_gattn_and_autograd(D, C, HC, N):
    case = R.dense_case(D, C, HC, N)
    # the reference's mask weighting mean(loss * mask / mean(mask)) == sum over the mask / count: row_weight = 1 / count,
    # rounded to fp32 in the C ABI -- hand the oracle's normaliser the same rounded weight by rescaling
    ref = R.multilabel_ref(**case)
    logits, loss, dl, dZ, dWc, dbc = _torch_oracle(case)
    scale = R.f32s(case["row_weight"]) * int((case["mask"] != 0).sum())      # 1 up to the rounding of the weight
    tol = dict(rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(ref.logits, logits.numpy(), **tol)
    np.testing.assert_allclose(ref.loss, loss * scale, **tol)
    np.testing.assert_allclose(ref.dl, dl.numpy() * scale, **tol)
    np.testing.assert_allclose(ref.dZ, dZ.numpy() * scale, **tol)
    np.testing.assert_allclose(ref.dWc, dWc.numpy() * scale, **tol)
    np.testing.assert_allclose(ref.dbc, dbc.numpy() * scale, **tol)
    assert not ref.dZ[~ref.live].any() and not ref.dl[~ref.live].any()


@pytest.mark.parametrize("D,C,HC,N", [(64, 8, 2, 257), (128, 33, 1, 65), (64, 100, 1, 63)])
def test_reference_agrees_with_micro_f1(D, C, HC, N):
    case = R.dense_case(D, C, HC, N)
    ref = R.multilabel_ref(**case)
    assert ref.undecided == 0 and ref.tp > 0
    f1 = BaseGAttN.micro_f1(torch.tensor(ref.logits), torch.tensor(case["y"]), torch.tensor(case["mask"] != 0))
    assert float(f1) == float(np.float32(ref.f1))
    assert ref.tp + ref.fn == int(case["y"][ref.live].sum())


def test_micro_f1_is_nan_without_a_true_positive():
    case = R.zero_case(64, 4, 1)
    ref = R.multilabel_ref(**case)
    assert ref.tp == 0 and ref.fp == 0 and ref.fn == int(case["y"][0].sum()) and math.isnan(ref.f1)
    assert ref.undecided == 0 and not ref.logits[0].any()
    assert abs(ref.loss - math.log(2.0)) < 1e-15
    assert R.f1_matches(float("nan"), ref) and not R.f1_matches(0.0, ref)


@pytest.mark.parametrize("C", [1, 3, 16, 17, 63, 64, 65, 100])
def test_pack_label_bits_round_trips(C):
    rng = np.random.default_rng(C)
    y = (rng.random((37, C)) < 0.5).astype(np.uint8)
    y[0], y[1] = 0, 1                      # no bit, every bit (bit 63 is the stored word's sign)
    for t in (torch.from_numpy(y), torch.from_numpy(y).bool(), torch.from_numpy(y).float()):
        w = ops.pack_label_bits(t)
        assert w.dtype == torch.int64 and tuple(w.shape) == (37, (C + 63) // 64) and w.is_contiguous()
        assert np.array_equal(w.numpy().view(np.uint64), R.pack_bits(y))
        assert np.array_equal(ops.unpack_label_bits(w, C).numpy(), y)
    for c in range(C):                     # class c is bit c % 64 of word c / 64
        assert np.array_equal((w.numpy().view(np.uint64)[:, c // 64] >> np.uint64(c % 64)) & np.uint64(1), y[:, c])
    with pytest.raises(ValueError):
        ops.pack_label_bits(torch.from_numpy(y.astype(np.int64) * 2))
    with pytest.raises(ValueError):
        ops.pack_label_bits(torch.from_numpy(y[:, 0]))


def test_ops_entry_has_no_cpu_path():
    case = R.dense_case(64, 3, 1, 15)
    t = {k: torch.from_numpy(case[k]) for k in ("Z", "Wc", "bc", "mask")}
    with pytest.raises(ValueError, match="GPU"):
        ops.classifier_multilabel(t["Z"], t["Wc"], t["bc"], ops.pack_label_bits(torch.from_numpy(case["y"])), t["mask"], 1.0)


def _trainer_args(c=3):
    from han_amd.gat import HeteGAT_multi
    wl = synth.make_workload("tiny")
    model = HeteGAT_multi().build(wl["p"], wl["f"], c, (8,), (8, 1), 16, device="cpu")
    return model, wl


def test_trainer_objective_checks():
    from han_amd.dist import NodePartition
    from han_amd.minibatch import MiniBatchTrainer
    from han_amd.trainer import HANTrainer, check_objective
    model, wl = _trainer_args()
    n = wl["n"]
    y = synth.multilabel_labels(wl["labels"], 3, seed=1)
    xs = [wl["x"]] * wl["p"]
    with pytest.raises(NotImplementedError, match="partition"):
        HANTrainer(model, xs, wl["graphs"], y, wl["train_mask"], part=NodePartition(n, 0, 2), objective="sigmoid")
    for bad in (wl["labels"], y[:, :2], y.unsqueeze(0)):
        with pytest.raises(ValueError, match="multi-hot"):
            HANTrainer(model, xs, wl["graphs"], bad, wl["train_mask"], objective="sigmoid")
        with pytest.raises(ValueError, match="multi-hot"):
            MiniBatchTrainer(model, xs, wl["graphs"], bad, wl["train_mask"], objective="sigmoid")
    with pytest.raises(ValueError, match="objective"):
        HANTrainer(model, xs, wl["graphs"], wl["labels"], wl["train_mask"], objective="hinge")
    check_objective("softmax", wl["labels"], 3, True)      # the single-label objective keeps working under a partition
    check_objective("sigmoid", y, 3)


def test_synth_multilabel_labels():
    com = torch.arange(4000) % 4
    y = synth.multilabel_labels(com, 5, seed=3)
    assert tuple(y.shape) == (4000, 5) and y.dtype == torch.uint8 and set(y.unique().tolist()) == {0, 1}
    assert torch.equal(y, synth.multilabel_labels(com, 5, seed=3))
    assert not torch.equal(y, synth.multilabel_labels(com, 5, seed=4))
    per = torch.stack([y[com == k].float().mean(0) for k in range(4)])      # plane frequencies per community
    assert bool(((per < 0.1) | (per > 0.9)).all()), "a plane is on or off per community, up to the 5 % flips"
    assert len({tuple((r > 0.5).tolist()) for r in per}) > 1, "the communities differ in their planes"
    assert bool((y.sum(1) > 1).any()), "some node carries several labels"


# ------------------------------------------------------------------ preconditions of the inputs shared with the GPU file
@pytest.mark.parametrize("D,C,HC", R.CELLS)
def test_planted_cases_are_decided(D, C, HC):
    case = R.planted_case(D, C, HC)
    ref = R.multilabel_ref(**case)
    N, rpb = R.loop_n(D, C), R.rows_per_block(D, C)
    assert ref.undecided == 0 and ref.T == R.N_LIVE and ref.N == N == R.GRID_CAP * rpb + 77
    on = np.nonzero(case["mask"])[0]
    assert on[0] == 0 and on[-1] == N - 1 and (on >= R.GRID_CAP * rpb).sum() >= 4
    assert (case["y"][on].sum(1) == 0).any() and (case["y"][on].sum(1) == C).any()
    assert np.isfinite(ref.logits).all() and np.abs(ref.logits[~ref.live]).max() > 1e3      # large finite junk
    assert ref.tp > 0 and ref.fp > 0 and ref.fn > 0
    if D in (64, 128) and C <= 64:
        rows, Zn = R.live_list(case)
        assert (np.diff(rows) > 0).all() and rows.size == 2 * R.N_LIVE and np.isnan(Zn).any()
        lref = R.multilabel_ref(**{**case, "Z": Zn}, rows=rows)
        assert np.array_equal(lref.counts, ref.counts) and lref.loss == ref.loss and lref.undecided == 0


@pytest.mark.parametrize("N", R.SMALL_N)
@pytest.mark.parametrize("D,C,HC", R.SMALL_CELLS)
def test_dense_cases_are_decided(D, C, HC, N):
    ref = R.multilabel_ref(**R.dense_case(D, C, HC, N))
    assert ref.undecided == 0 and ref.T >= 1


@pytest.mark.parametrize("s", [80.0, 1.0e4])
def test_saturation_case_reference(s):
    case = R.saturation_case(64, 4, s)
    ref = R.multilabel_ref(**case)
    assert np.array_equal(np.abs(ref.logits), np.full_like(ref.logits, s)) and ref.undecided == 0
    assert np.isfinite(ref.loss) and np.isfinite(ref.dZ).all()
    # rows 0 mod 4 carry their own predictions: sigma - y is 0 for the positive logits and exp(-s) for the negative ones
    assert np.abs(ref.dl[0::4]).max() <= 0.125 / 4 * math.exp(-s)
    # rows 1 mod 4 carry the opposite: every class adds (w / C) (+-1) (+-1) = w / C, C of them
    assert np.array_equal(ref.dZ[1::4, 0], np.full(4, 0.125))


def test_big_count_is_odd_and_past_2_24():
    assert R.BIG_N * R.BIG_C == R.BIG_TP and R.BIG_TP % 2 == 1 and R.BIG_TP > 2 ** 24
    assert float(np.float32(R.BIG_TP)) != R.BIG_TP


def test_pack_label_bits_in_row_chunks(monkeypatch):
    y = torch.from_numpy((np.random.default_rng(2).random((101, 70)) < 0.5).astype(np.uint8))
    whole = ops.pack_label_bits(y)
    monkeypatch.setattr(ops, "PACK_ROWS", 16)      # 7 steps, the last one short
    assert torch.equal(ops.pack_label_bits(y), whole)
    assert np.array_equal(whole.numpy().view(np.uint64), R.pack_bits(y.numpy()))


def _stopper(kind):
    """The state early_stopping works on, without a graph or a device."""
    import types
    from han_amd.minibatch import MiniBatchTrainer
    from han_amd.trainer import HANTrainer
    cls = HANTrainer if kind == "full" else MiniBatchTrainer
    s = types.SimpleNamespace(vlss_mn=float("inf"), vacc_mx=0.0, curr_step=0, patience=3, best_state=None,
                              overlap_eval=False, _flat_prev=None, model=types.SimpleNamespace(flat=torch.zeros(4)))
    return s, lambda vl, va: cls.early_stopping(s, vl, va)


@pytest.mark.parametrize("kind", ["full", "minibatch"])
def test_early_stopping_survives_a_nan_micro_f1(kind):
    """tp == 0 gives a NaN micro-F1 in the first epochs of rare labels: it is no improvement, it is not stored, and the
    first real value afterwards is an improvement and saves the weights."""
    s, step = _stopper(kind)
    nan = float("nan")
    assert step(0.9, nan) is False                 # the loss improved: the patience starts over, nothing is saved
    assert s.vacc_mx == 0.0 and s.vlss_mn == 0.9 and s.best_state is None and s.curr_step == 0
    assert step(0.8, nan) is False and s.vacc_mx == 0.0 and s.best_state is None
    s.model.flat.fill_(1.0)
    assert step(0.7, 0.4) is False                 # better loss, first real F1: saved
    assert s.vacc_mx == 0.4 and s.vlss_mn == 0.7 and torch.equal(s.best_state, torch.ones(4))
    s.model.flat.fill_(2.0)
    assert step(0.6, nan) is False and s.vacc_mx == 0.4 and torch.equal(s.best_state, torch.ones(4))
    assert step(0.5, 0.5) is False and torch.equal(s.best_state, torch.full((4,), 2.0)) and s.vacc_mx == 0.5
    # neither improves, NaN included: the patience runs out
    assert step(0.9, nan) is False and step(0.9, 0.1) is False and step(0.9, nan) is True


@pytest.mark.parametrize("kind", ["full", "minibatch"])
def test_early_stopping_without_nan_is_the_reference_rule(kind):
    s, step = _stopper(kind)
    assert step(1.0, 0.3) is False and s.best_state is not None and (s.vacc_mx, s.vlss_mn) == (0.3, 1.0)
    s.model.flat.fill_(1.0)
    assert step(0.9, 0.2) is False and (s.vacc_mx, s.vlss_mn, s.curr_step) == (0.3, 0.9, 0)
    assert not s.best_state.any()                  # only one of the two improved: no snapshot
    assert step(1.1, 0.3) is False and s.curr_step == 0 and not s.best_state.any()      # ">=" on the metric
    assert step(1.1, 0.1) is False and s.curr_step == 1


def test_multilabel_result_is_a_three_tuple_with_counts():
    from han_amd import layers
    t = [torch.tensor(float(i)) for i in range(3)]
    counts = torch.tensor([3, 1, 2])
    r = layers.MultiLabelResult(*t, counts)
    loss, f1, logits = r
    assert len(r) == 3 and tuple(r) == tuple(t) and r[2] is logits and r.counts is counts
    assert r.loss is loss and r.micro_f1 is f1 and r.logits is logits
    with pytest.raises(IndexError):
        r[3]
    assert float(layers.micro_f1_of_counts(counts)) == float(np.float32(6.0 / 9.0))
    assert math.isnan(float(layers.micro_f1_of_counts(torch.tensor([0, 5, 0]))))
    assert math.isnan(float(layers.micro_f1_of_counts(torch.tensor([0, 0, 0]))))
