"""han_project_fwd_both: the training forward and the eval forward of K1 in one pass over X.

Both row sets must carry the BYTES of the two separate calls: the training H / f1 / f2 / keep table those of
project_fwd_multi with the same seeds and dropout rates, the eval H / f1 / f2 those of project_fwd_multi without
dropout.  The shapes are the smallest at which the kernel can still go wrong: the first row count with a keep table
(32 768 = 256 blocks of 128 rows) and one that leaves a partial last block; F = 8 (a lone partial K-step), 40 (a
partial second K-step), 136 (one full keep-line flush plus a partial group) and 256 (the bench width)."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

P = 2
NOT_ELIGIBLE = -4
SEEDS = ((0x1234567, 0x89ABCDEF01), (3, 2 ** 63 + 11))
ROW_OFFSETS = (0, 1_000_003)


def _bits(t):
    return t.view(torch.uint8) if t.dtype == torch.uint8 else t.contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


_inputs = {}


def _case(dev, n, f, p=P):
    """X, the parameters and the eval reference of one shape, made once and never written again."""
    key = (n, f, p)
    if key not in _inputs:
        from han_amd import ops
        g = torch.Generator(device=dev).manual_seed(1000 * f + n % 1000 + p)
        rnd = lambda *s: torch.randn(s, device=dev, generator=g)
        prm = (rnd(p, f, 64) * 0.1, rnd(p, 8, 8), rnd(p, 8, 8), rnd(p, 8), rnd(p, 8))
        X = rnd(n, f)
        _inputs[key] = (X, prm, ops.project_fwd_multi(X, *prm))
    return _inputs[key]


@pytest.mark.parametrize("drops", [(0.6, 0.6), (0.6, 0.0)], ids=["in06_fts06", "in06_fts0"])
@pytest.mark.parametrize("f", [8, 40, 136, 256])
@pytest.mark.parametrize("n", [32768, 32768 + 72])
def test_both_row_sets_carry_the_bytes_of_the_separate_calls(dev, n, f, drops):
    from han_amd import ops
    X, prm, ev_ref = _case(dev, n, f)
    assert ops.keep_bytes(n, f, f) == n * f + 128
    for seeds in SEEDS:
        for ro in ROW_OFFSETS:
            got = ops.project_fwd_both(X, *prm, drops[0], drops[1], seeds, row_offset=ro)
            assert got is not None, "eligible shape declined"
            (H, f1, f2, keep), (He, f1e, f2e) = got
            rH, rf1, rf2, rkeep = ops.project_fwd_multi(X, *prm, in_drop=drops[0], fts_drop=drops[1], seeds=seeds,
                                                        row_offset=ro, want_keep=True)
            what = f"seeds={seeds} row_offset={ro}"
            assert _same(H, rH), f"training H differs ({what})"
            assert _same(f1, rf1) and _same(f2, rf2), f"training scores differ ({what})"
            for p in range(P):      # the last 128 bytes of a table are slack for whole-tile loads: never written
                assert _same(keep[p][:n * f], rkeep[p][:n * f]), f"keep table {p} differs ({what})"
            assert _same(He, ev_ref[0]), f"eval H differs ({what})"
            assert _same(f1e, ev_ref[1]) and _same(f2e, ev_ref[2]), f"eval scores differ ({what})"


@pytest.mark.parametrize("n,f,p", [(32768, 64, 3), (32768, 12, 2), (32767, 64, 2)], ids=["P3", "F12", "N32767"])
def test_ineligible_shapes_are_declined_before_any_launch(dev, n, f, p):
    from han_amd import _lib, ops
    lib = _lib.load()
    X, prm, _ = _case(dev, n, f, p)
    assert ops.project_fwd_both(X, *prm, 0.6, 0.6, list(range(1, p + 1))) is None
    # the C call itself, on outputs that hold a pattern: the code, and not a byte written
    outs = [torch.full(s, 7.25, device=dev) for s in ((p, n, 64), (p, n, 8), (p, n, 8)) * 2]
    keep = torch.full((p, n * f + 128), 0x5A, dtype=torch.uint8, device=dev)
    ws = torch.full((1 << 20,), 0x5A, dtype=torch.uint8, device=dev)
    seeds = (ctypes.c_uint64 * p)(*range(1, p + 1))
    H, f1, f2, He, f1e, f2e = outs
    rc = lib.han_project_fwd_both(X.data_ptr(), 0, f, *[t.data_ptr() for t in prm], H.data_ptr(), 0, f1.data_ptr(),
                                  f2.data_ptr(), He.data_ptr(), f1e.data_ptr(), f2e.data_ptr(), ws.data_ptr(), ws.numel(),
                                  n, f, 8, 8, p, 0.6, 0.6, seeds, None, 0, keep.data_ptr(), 0, None)
    torch.cuda.synchronize()
    assert rc == NOT_ELIGIBLE
    assert all(bool((t == 7.25).all()) for t in outs)
    assert bool((keep == 0x5A).all()) and bool((ws == 0x5A).all())


# ------------------------------------------------------------------------------------------------ the trainer
_wl = {}


def _workload(dev):
    if not _wl:
        from han_amd import synth
        n = 32768
        _wl["wl"] = synth.planted_partition(n, 4, P, 64, deg_in=6, deg_out=2, noise=1.0, seed=3, device=dev)
        u = torch.rand(n, generator=torch.Generator().manual_seed(1))
        _wl["masks"] = ((u < 0.1).to(torch.uint8).to(dev), ((u >= 0.1) & (u < 0.2)).to(torch.uint8).to(dev))
    return _wl["wl"], _wl["masks"]


def _run(dev, shared, writes=()):
    """Epochs from the seeds every run shares; writes: per epoch after which it happens, how one parameter is written.
    -> (scalars of every epoch, model.flat, model.flat_grad, training forwards served from a stash)."""
    from han_amd import rng as hrng
    from han_amd.gat import HeteGAT_multi
    from han_amd.trainer import HANTrainer
    wl, masks = _workload(dev)
    torch.manual_seed(0)
    hrng.manual_seed(5)
    model = HeteGAT_multi().build(P, 64, 4, (8,), (8, 1), 128, device=dev, generator=torch.Generator().manual_seed(11))
    tr = HANTrainer(model, [wl["x"]] * P, wl["graphs"], wl["labels"], masks[0], masks[1], shared_projection=shared)
    assert tr.shared_projection is bool(shared)
    scalars = []
    for ep in range(3):
        scalars.append(torch.stack([v.reshape(()) for v in tr.epoch()]).clone())
        how = dict(writes).get(ep)
        if how == "state_dict":      # the public state-loading path
            sd = {k: v.clone() for k, v in model.state_dict().items()}
            sd["W"][1, 3, 5] += 0.125
            model.load_state_dict(sd)
        elif how == "flat":
            new = model.flat.clone()
            new[7] -= 0.25
            model.flat.copy_(new)
    torch.cuda.synchronize()
    taken = model.shared_proj.taken if model.shared_proj is not None else 0
    return torch.stack(scalars), model.flat.clone(), model.flat_grad.clone(), taken


_plain = {}


def _reference(dev, writes):
    if writes not in _plain:
        _plain[writes] = _run(dev, False, writes)
    return _plain[writes]


def test_trainer_epochs_are_byte_equal_with_and_without_the_shared_projection(dev):
    s0, p0, g0, t0 = _reference(dev, ())
    s1, p1, g1, t1 = _run(dev, True)
    assert (t0, t1) == (0, 2), "the training forwards of epochs 2 and 3 run from the stash"
    assert _same(s1, s0), (s1, s0)
    assert _same(p1, p0) and _same(g1, g0)


@pytest.mark.parametrize("how", ["state_dict", "flat"])
def test_a_parameter_write_between_two_epochs_drops_the_stash(dev, how):
    writes = ((0, how),)
    s0, p0, g0, _ = _reference(dev, writes)
    s1, p1, g1, taken = _run(dev, True, writes)
    assert taken == 1, "epoch 2 must project again after the write, epoch 3 runs from the stash"
    assert _same(s1, s0), (s1, s0)
    assert _same(p1, p0) and _same(g1, g0)
    assert not _same(p0, _reference(dev, ())[1]), "the write must matter"


def test_shared_projection_true_raises_where_it_cannot_act(dev):
    from han_amd.gat import HeteGAT_multi
    from han_amd.trainer import HANTrainer
    wl, masks = _workload(dev)
    model = HeteGAT_multi().build(P, 64, 4, (8,), (8, 1), 128, device=dev, generator=torch.Generator().manual_seed(11))
    with pytest.raises(ValueError, match="shared_projection"):
        HANTrainer(model, [wl["x"]] * P, wl["graphs"], wl["labels"], masks[0], masks[1], shared_projection=True, ffd_drop=0.0)
    with pytest.raises(ValueError, match="shared_projection"):
        HANTrainer(model, [wl["x"]] * P, wl["graphs"], wl["labels"], masks[0], masks[1], shared_projection="yes")
    tr = HANTrainer(model, [wl["x"]] * P, wl["graphs"], wl["labels"], masks[0], masks[1], shared_projection=True)
    tr.epoch()
    assert model.shared_proj._stash is not None
    tr.eval_step()          # a bare eval_step() neither uses nor disturbs it
    assert model.shared_proj._stash is not None and model.shared_proj.armed is None
    tr.restore_best()       # (no best state yet: nothing written, nothing dropped)
    tr.best_state = model.flat.clone()
    tr.restore_best()
    assert model.shared_proj._stash is None
