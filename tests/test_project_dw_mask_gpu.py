"""dW through the keep table (project_bwd_blk_kernel, han_amd/csrc/project.hip) at the smallest shapes where its
scalar keep-word loads can go wrong.

The table exists from N = 32768, so N = 32768, +1, +31, +33 cover a whole last tile, the ragged last tile, the ragged
last chunk and the row clamp of the loads requested ahead; F = 8 (one octet: waves 1-3 lie wholly beyond F and the
last row's loads reach into the slack), F = 40 (a wave straddles F), F = 136 (a second feature block of 8 features)
and F = 256.  Every case: the table the forward wrote must give the dW of the hash-regenerating kernel bit for bit,
and both must lie within the float64 bound of tests/k1_cases.py (random inputs, keep probability 0.4)."""
import functools

import numpy as np
import pytest
import torch

from tests import k1_cases as kc

pytestmark = pytest.mark.gpu

NS = (32768, 32769, 32768 + 31, 32768 + 33)
FS = (8, 40, 136, 256)


def _case(n, f, **kw):
    return kc.Case("dw", n, f, drop=0.6, keep_table=True, random=True, **kw)


CASES = [_case(n, f) for n in NS for f in FS] + [
    _case(32769, 40, view="slice"),                       # ldx = F + 8 > F
    _case(32768 + 31, 136, row_offset=kc.BIG_OFFSET),
    _case(32768 + 33, 256, xbf=True),
]


@functools.lru_cache(maxsize=None)
def _problem(c):
    """inputs and the float64 reference of a case, computed once and never written to"""
    x, dH = kc.make_inputs(c)
    ref, S = kc.dw_reference(x, dH, c.K, c.FP, c.drop, c.eff_seed, c.row_offset)
    for a in (x, dH, ref, S):
        a.setflags(write=False)
    return x, dH, ref, S


def _kw(c):
    return dict(in_drop=c.drop, seed=c.seed, row_offset=c.row_offset)


def _table(ops, dev, c, xt):
    """the keep table of the training forward on xt (the projection's own outputs are not looked at)"""
    rng = np.random.default_rng(c.f)
    W = kc._t(kc._ints(rng, (c.f, kc.D), 1), dev)
    a, b = kc._t(kc._ints(rng, (8, 8), 1), dev), kc._t(kc._ints(rng, (8,), 1), dev)
    keep = ops.project_fwd(xt, W, a, a, b, b, want_keep=True, **_kw(c))[3]
    assert keep is not None and keep.numel() == c.n * c.f + 128
    return keep


def _within_bound(c, got, ref, S, name):
    err = np.abs(kc._f64(got) - ref)
    tol = kc.bound(c.n, S, c)
    assert (err <= tol).all(), (name, float((err / np.maximum(tol, 1e-300)).max()))


@pytest.mark.parametrize("c", CASES, ids=kc.ids(CASES))
def test_dw_keep_table_equals_regenerated_draws(dev, c):
    from han_amd import ops
    x, dH, ref, S = _problem(c)
    xt, dHt = kc.x_tensor(x, dev, c), kc._t(dH, dev)
    if c.view:
        assert xt.stride(0) > c.f
    keep = _table(ops, dev, c, xt)
    dW = ops.project_bwd(xt, dHt, c.K, c.FP, **_kw(c))
    dWk = ops.project_bwd(xt, dHt, c.K, c.FP, keep=keep, **_kw(c))
    torch.cuda.synchronize()
    assert torch.equal(dWk, dW)
    _within_bound(c, dW, ref, S, "dW from regenerated draws")
    _within_bound(c, dWk, ref, S, "dW through the keep table")


def test_dw_inf_in_elements_every_head_drops(dev):
    """An element that all eight heads drop is selected away, not multiplied by zero: inf there must not reach dW."""
    from han_amd import ops
    c = _case(32768 + 33, 40)
    x, dH, ref, S = _problem(c)
    dropped = ~kc.seq_masks(c.eff_seed, 0, c.n, c.f, c.K, c.drop, c.row_offset).any(axis=0)      # (n, f)
    assert dropped.sum() >= 100                     # 0.6^8 = 1.7 % of the elements
    xi = x.copy()
    xi[dropped] = np.inf
    x0 = x.copy()
    x0[dropped] = 0.0
    ref0, S0 = kc.dw_reference(x0, dH, c.K, c.FP, c.drop, c.eff_seed, c.row_offset)
    xt, dHt = kc.x_tensor(xi, dev, c), kc._t(dH, dev)
    assert int(torch.isinf(xt).sum()) == int(dropped.sum())
    keep = _table(ops, dev, c, xt)
    dW = ops.project_bwd(xt, dHt, c.K, c.FP, **_kw(c))
    dWk = ops.project_bwd(xt, dHt, c.K, c.FP, keep=keep, **_kw(c))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dWk).all())
    assert torch.equal(dWk, dW)
    _within_bound(c, dWk, ref0, S0, "dW through the keep table")


@pytest.mark.parametrize("f", (8, 136))
def test_dw_ignores_bytes_beyond_the_table_rows(dev, f):
    """Nothing read beyond F may reach a result: the 128 bytes of slack and the tables of the neighbouring allocations
    (P tables lie han_project_keep_bytes() apart) filled with 0xFF and with 0x00 give the same dW."""
    from han_amd import ops
    c = _case(32768 + 33, f)
    x, dH, ref, S = _problem(c)
    xt, dHt = kc.x_tensor(x, dev, c), kc._t(dH, dev)
    keep = _table(ops, dev, c, xt)
    kb, used = keep.numel(), c.n * c.f
    got = []
    for fill in (0xFF, 0x00):
        three = torch.full((3 * kb,), fill, dtype=torch.uint8, device=dev)
        mid = three[kb:2 * kb]
        assert mid.data_ptr() % 8 == 0
        mid[:used] = keep[:used]
        got.append(ops.project_bwd(xt, dHt, c.K, c.FP, keep=mid, **_kw(c)))
    torch.cuda.synchronize()
    assert torch.equal(got[0], got[1])
    assert torch.equal(got[0], ops.project_bwd(xt, dHt, c.K, c.FP, **_kw(c)))
    _within_bound(c, got[0], ref, S, "dW through the keep table")
