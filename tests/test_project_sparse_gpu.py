"""K1 sparse on the GPU: han_project_sparse_fwd / han_project_sparse_bwd through han_amd.ops, and sparse features
through the model and the trainer.

The reference is NumPy float64 on the densified matrix with the dropout masks of tests/rng_ref.py -- never the
sparse kernels themselves.  Tolerances are the project's: 1e-4 absolute on forward values against
float64, 2e-3 relative to the largest element on gradients, 2e-4 on parameters after three training steps."""
import functools

import numpy as np
import pytest
import torch

from han_amd import SparseFeatures, ops, synth
from han_amd import rng as hrng
from tests import k1_cases as kc
from tests import rng_ref
from tests.helpers import rel_err

pytestmark = pytest.mark.gpu

TOL, GTOL, PTOL = 1e-4, 2e-3, 2e-4
SHAPES = [(8, 8), (16, 4), (4, 16), (2, 32), (1, 64)]
SEED = 0x1234_5678_9ABC_DEF1
N, F = 67, 37


def _t(a, dev, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype, device=dev)


@functools.lru_cache(maxsize=None)
def _matrix(binary: bool):
    """(rowptr, colidx, values or None, dense float64) of the 67 x 37 matrix: row 0 empty, row 1 one entry, row 2
    full, a stored zero at (3, 5) (with values; the binary form stores a 1 there)."""
    rng = np.random.default_rng(11)
    pat = rng.random((N, F)) < 0.15
    pat[0] = False
    pat[1] = False
    pat[1, 30] = True
    pat[2] = True
    pat[3, 5] = True
    vals = rng.standard_normal((N, F)) * pat
    vals[3, 5] = 0.0
    rowptr = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(pat.sum(1), out=rowptr[1:])
    colidx = np.nonzero(pat)[1].astype(np.int32)
    if binary:
        return rowptr, colidx, None, pat.astype(np.float64)
    v32 = vals[pat].astype(np.float32)
    dense = np.zeros((N, F))
    dense[pat] = v32
    return rowptr, colidx, v32, dense


def _features(binary, dev):
    rowptr, colidx, vals, dense = _matrix(binary)
    sf = SparseFeatures.from_arrays(rowptr, colidx, vals, F, device=dev)
    assert sf.nnz == len(colidx) and (sf.values is None) == binary      # the stored zero is kept
    return sf, dense


@functools.lru_cache(maxsize=None)
def _params(K, FP, f=F):
    rng = np.random.default_rng(100 + K)
    r32 = lambda *s: (rng.standard_normal(s) * 0.5).astype(np.float32)
    return r32(f, 64), r32(K, FP), r32(K, FP), r32(K), r32(K)


def _ref_fwd(dense, W, a1, a2, b1, b2, K, FP, in_drop=0.0, seed=0, row_offset=0):
    """float64 H (N,64), f1, f2 (N,K) of utils/layers.py:18-24 with the kernels' input-dropout draws."""
    n, f = dense.shape
    W, a1, a2, b1, b2 = (np.asarray(v, dtype=np.float64) for v in (W, a1, a2, b1, b2))
    H = np.zeros((n, 64))
    if in_drop > 0:
        mask = rng_ref.seq_mask(seed, n, f, K, in_drop, row_offset)
        keep = rng_ref.keep_prob32(in_drop)
    for k in range(K):
        c = slice(k * FP, (k + 1) * FP)
        H[:, c] = (dense * mask[k] / keep if in_drop > 0 else dense) @ W[:, c]
    Hk = H.reshape(n, K, FP)
    return H, (Hk * a1[None]).sum(-1) + b1, (Hk * a2[None]).sum(-1) + b2


def _run_fwd(sf, K, FP, dev, **kw):
    W, a1, a2, b1, b2 = (_t(v, dev) for v in _params(K, FP, sf.shape[1]))
    return ops.project_fwd(sf, W, a1, a2, b1, b2, **kw)


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("binary", [False, True])
@pytest.mark.parametrize("K,FP", SHAPES)
def test_forward_no_dropout(dev, K, FP, binary):
    sf, dense = _features(binary, dev)
    H, f1, f2 = _run_fwd(sf, K, FP, dev)
    Hr, f1r, f2r = _ref_fwd(dense, *_params(K, FP), K, FP)
    for got, ref, name in ((H, Hr, "H"), (f1, f1r, "f1"), (f2, f2r, "f2")):
        err = np.abs(got.cpu().numpy() - ref).max()
        print(f"{name} ({K},{FP}) binary={binary}: max abs err {err:.3e}")
        assert err < TOL, name
    b1, b2 = _params(K, FP)[3:]
    assert np.array_equal(f1[0].cpu().numpy(), b1) and np.array_equal(f2[0].cpu().numpy(), b2)      # the empty row
    assert not H[0].any()


# ------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("K,FP", [(8, 8), (1, 64)])
def test_forward_with_dropout(dev, K, FP):
    drop, off = 0.6, 1000
    sf, dense = _features(False, dev)
    kw = dict(in_drop=drop, fts_drop=drop, row_offset=off)
    H, f1, f2 = _run_fwd(sf, K, FP, dev, seed=SEED, **kw)
    Hr, f1r, f2r = _ref_fwd(dense, *_params(K, FP), K, FP, drop, SEED, off)
    for got, ref, name in ((H, Hr, "H"), (f1, f1r, "f1"), (f2, f2r, "f2")):
        err = np.abs(got.cpu().numpy() - ref).max()
        print(f"{name} ({K},{FP}) dropout: max abs err {err:.3e}")
        assert err < TOL, name
    bits = (H.view(torch.int32) & 1).cpu().numpy()
    assert np.array_equal(bits, rng_ref.fts_mask(SEED, N, 64, drop, off).astype(np.int32))
    again = _run_fwd(sf, K, FP, dev, seed=SEED, **kw)
    assert all(torch.equal(a, b) for a, b in zip((H, f1, f2), again))
    other = _run_fwd(sf, K, FP, dev, seed=SEED + 1, **kw)
    assert not torch.equal(other[0], H)
    # a device seed word (a captured step): the effective seed is splitmix64(seed + word)
    word = 0x0123_4567_89AB
    with_dev = _run_fwd(sf, K, FP, dev, seed=SEED, seed_dev=torch.tensor([word], dtype=torch.int64, device=dev), **kw)
    eff = rng_ref.resolve_seed(SEED, word)
    resolved = _run_fwd(sf, K, FP, dev, seed=eff, **kw)
    assert all(torch.equal(a, b) for a, b in zip(with_dev, resolved))
    assert not torch.equal(with_dev[0], H)
    assert np.array_equal((with_dev[0].view(torch.int32) & 1).cpu().numpy(),
                          rng_ref.fts_mask(eff, N, 64, drop, off).astype(np.int32))
    # column slice 1 of a wide head draws its projected-row dropout from its own stream
    sl = _run_fwd(sf, K, FP, dev, seed=SEED, flags=ops.flag_fts_slice(1), **kw)
    assert np.array_equal((sl[0].view(torch.int32) & 1).cpu().numpy(),
                          rng_ref.fts_mask(SEED, N, 64, drop, off, slice_index=1).astype(np.int32))
    assert np.abs(sl[0].cpu().numpy() - Hr).max() < TOL


# ------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("drop", [0.0, 0.6])
@pytest.mark.parametrize("binary", [False, True])
def test_forward_bf16_table(dev, drop, binary):
    K, FP, off = 8, 8, 1000 if drop else 0
    sf, dense = _features(binary, dev)
    H, f1, f2 = _run_fwd(sf, K, FP, dev, in_drop=drop, fts_drop=drop, seed=SEED, row_offset=off,
                         table_dtype=torch.bfloat16)
    assert H.dtype == torch.bfloat16
    W, a1, a2, b1, b2 = _params(K, FP)
    Hr, _, _ = _ref_fwd(dense, W, a1, a2, b1, b2, K, FP, drop, SEED, off)
    Hs = H.float().cpu().numpy().astype(np.float64)      # the rows as stored
    # rounding to nearest is <= 2^-8 relative, the stamped bit <= 2^-7
    used = (np.abs(Hs - Hr) / (2.0 ** -6 * np.abs(Hr) + 1e-4)).max()
    print(f"bf16 drop={drop} binary={binary}: largest error / bound {used:.3f}")
    assert used < 1
    if drop:
        bits = (H.view(torch.int16).to(torch.int32) & 1).cpu().numpy()
        assert np.array_equal(bits, rng_ref.fts_mask(SEED, N, 64, drop, off).astype(np.int32))
    Hk = Hs.reshape(N, K, FP)
    for got, a, b in ((f1, a1, b1), (f2, a2, b2)):
        ref = (Hk * a.astype(np.float64)[None]).sum(-1) + b.astype(np.float64)
        assert np.abs(got.cpu().numpy() - ref).max() < 1e-5


# ------------------------------------------------------------------------------------------------ 3b
@functools.lru_cache(maxsize=None)
def _grid_problem(f, path, K, FP, bf16_table):
    """An exact-grid forward case of tests/k1_cases.py (its generators and units) with about 5 % of X kept and two
    score coefficients per head: the CSR triple, the dense matrix and the parameters, as float64 arrays holding exactly
    the values the kernels get."""
    c = kc.Case("fwd", 130, f, path, K=K, FP=FP, drop=0.5, fts=0.5, bf16_table=bf16_table, row_offset=1000)
    x, W, a1, a2, b1, b2 = kc.fwd_inputs(c)              # asserts the precondition for the full matrix
    pat = np.random.default_rng([c.n, f, 5]).random((c.n, f)) < 0.05
    pat[0] = False                                       # a row without entries
    x = x * pat
    # The scores are sums over the rows AS STORED, and a stamped keep bit takes an fp32 element one unit in its last
    # place off the grid: a sum of three or more such terms rounds differently in different orders (the tile form adds
    # a head's products in a tree over its lanes, the row form four per lane in sequence first).  Two coefficients per
    # head, each a power of two: every product is exact and a head's sum is ONE rounded addition, the same in any
    # order, so the equality asserted below holds for every kernel that keeps the contract.
    arng = np.random.default_rng([f, K, 7])
    for a in (a1, a2):
        kept = np.zeros((K, FP), dtype=bool)
        for k in range(K):
            kept[k, arng.choice(FP, 2, replace=False)] = True
        a[0] = np.where(kept, np.where(a[0] == 0, kc.GA, a[0]), 0.0)
        m = np.abs(a[0][kept]) / kc.GA
        assert ((a[0] != 0).sum(-1) == 2).all() and np.isin(m, (1, 2)).all()
    # the precondition of k1_cases.fwd_inputs again, for the matrix as used: in float64, from the inputs alone, all
    # keep draws taken as "kept" -- every product and partial sum of H, in any order, is an integer below 2^24 units
    S = 2 * (np.abs(x) @ np.abs(W[0])) / (kc.GX * kc.GW)
    assert S.max() < kc.TWO24 and np.array_equal(x, x.astype(np.float32).astype(np.float64))
    Sst = S * (1 + 2.0 ** -8) if bf16_table else S
    for a, b in ((a1, b1), (a2, b2)):
        sc = (Sst.reshape(c.n, K, FP) * np.abs(a[0] / kc.GA)).sum(-1) + np.abs(b[0]) / (kc.GX * kc.GW * kc.GA)
        assert sc.max() < kc.TWO24
    rowptr = np.zeros(c.n + 1, dtype=np.int64)
    np.cumsum(pat.sum(1), out=rowptr[1:])
    return c, rowptr, np.nonzero(pat)[1].astype(np.int32), x[pat].astype(np.float32), x, (W[0], a1[0], a2[0], b1[0], b2[0])


@pytest.mark.parametrize("bf16_table", [False, True], ids=["f32tab", "bf16tab"])
@pytest.mark.parametrize("K,FP", [(8, 8), (4, 16)])
@pytest.mark.parametrize("f,path", [(77, "plain"), (300, "split")])
def test_sparse_equals_dense_on_the_grid(dev, f, path, K, FP, bf16_table):
    """The stored-row contract across both lane layouts (han_k1_epilogue.h): on exact-grid inputs the CSR forward and
    the dense forward of the densified matrix -- F = 77: project_fwd_kernel, tile form; F = 300: split-F +
    project_finish_kernel, row form -- must store the same bits of H and the same f1 / f2, with both dropouts, a row
    offset and the keep bits of column slice 1.

    H is exact on the grid in any order; the score sums are made order-free by the inputs (_grid_problem: two
    power-of-two coefficients per head), since the stamped bits take fp32 elements off the grid.  With all F' coefficients
    of a head non-zero the two forms' scores differ in the last bits of about one in ten on the F = 77 route with an
    fp32 table (98 + 113 of 2 x 1040 scores at 8 x 8 on an MI355X, before and after the epilogue moved into the header):
    a property of the two summation orders, not of the contract."""
    c, rowptr, colidx, vals, dense, params = _grid_problem(f, path, K, FP, bf16_table)
    assert kc.forward_path(c.n, f) == path
    sf = SparseFeatures.from_arrays(rowptr, colidx, vals, f, device=dev)
    tdt = torch.bfloat16 if bf16_table else torch.float32
    W, a1, a2, b1, b2 = (_t(v, dev) for v in params)
    kw = dict(in_drop=c.drop, fts_drop=c.fts, seed=c.seed, row_offset=c.row_offset, table_dtype=tdt,
              flags=ops.flag_fts_slice(1))
    Hs, f1s, f2s = ops.project_fwd(sf, W, a1, a2, b1, b2, **kw)
    Hd, f1d, f2d = ops.project_fwd(_t(dense, dev), W, a1, a2, b1, b2, **kw)
    it = torch.int16 if bf16_table else torch.int32
    bits = (Hs.view(it).to(torch.int32) & 1).cpu().numpy()
    assert np.array_equal(bits, rng_ref.fts_mask(c.seed, c.n, 64, c.fts, c.row_offset, slice_index=1).astype(np.int32))
    diff = [int((a != b).sum()) for a, b in ((Hs.view(it), Hd.view(it)), (f1s, f1d), (f2s, f2d))]
    print(f"sparse vs dense {path} ({K},{FP}) {'bf16' if bf16_table else 'fp32'} table: "
          f"differing elements H {diff[0]} f1 {diff[1]} f2 {diff[2]}")
    assert Hs.any() and torch.equal(Hs.view(it), Hd.view(it))
    assert torch.equal(f1s, f1d) and torch.equal(f2s, f2d)
    # and both are the scores of the rows as stored: the head's two products (exact), one fp32 addition, then b
    st = Hs.float().cpu().numpy().reshape(c.n, K, FP)
    for got, a, b in ((f1s, params[1], params[3]), (f2s, params[2], params[4])):
        cols = np.argsort(a == 0, axis=-1, kind="stable")[:, :2]                  # the two kept columns of each head
        p = np.take_along_axis(st, cols[None].repeat(c.n, 0), -1) * np.take_along_axis(a, cols, -1).astype(np.float32)[None]
        want = ((p[..., 0] + p[..., 1]).astype(np.float32) + b.astype(np.float32)[None]).astype(np.float32)
        assert np.array_equal(got.cpu().numpy(), want) and (want != b.astype(np.float32)[None]).any()


# ------------------------------------------------------------------------------------------------ 4
@functools.lru_cache(maxsize=None)
def _dw_matrix():
    """N = 2 * SPARSE_COL_CHUNK + 3 rows: column 0 is stored in every row (three chunks, the last of three entries),
    column 7 is empty, column 9 has a single entry."""
    n = 2 * ops.SPARSE_COL_CHUNK + 3
    rng = np.random.default_rng(21)
    pat = rng.random((n, F)) < 0.1
    pat[:, 0] = True
    pat[:, 7] = False
    pat[:, 9] = False
    pat[n // 2, 9] = True
    v32 = rng.standard_normal((n, F)).astype(np.float32)
    dense = np.where(pat, v32, 0).astype(np.float64)
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(pat.sum(1), out=rowptr[1:])
    return rowptr, np.nonzero(pat)[1].astype(np.int32), v32[pat], dense, pat.astype(np.float64)


def _ref_dw(dense, dH, K, FP, in_drop, seed, row_offset):
    n, f = dense.shape
    dW = np.zeros((f, 64))
    if in_drop > 0:
        mask = rng_ref.seq_mask(seed, n, f, K, in_drop, row_offset)
        keep = rng_ref.keep_prob32(in_drop)
    for k in range(K):
        c = slice(k * FP, (k + 1) * FP)
        dW[:, c] = (dense * mask[k] / keep if in_drop > 0 else dense).T @ dH[:, c]
    return dW


@pytest.mark.parametrize("binary", [False, True])
@pytest.mark.parametrize("drop", [0.0, 0.6])
@pytest.mark.parametrize("K,FP", [(8, 8), (2, 32)])
def test_dw(dev, K, FP, drop, binary):
    rowptr, colidx, vals, dense, pat = _dw_matrix()
    n, off = dense.shape[0], 1000
    assert n == 2 * ops.SPARSE_COL_CHUNK + 3
    sf = SparseFeatures.from_arrays(rowptr, colidx, None if binary else vals, F, device=dev)
    t = sf.transposed()
    assert t["n_long"] == 1 and t["n_chunks"] == 3 and int(t["long_cols"][0]) == 0      # the chunk merge runs
    dH64 = np.random.default_rng(22).standard_normal((n, 64))
    dH = _t(dH64, dev)
    ref = _ref_dw(pat if binary else dense, dH.cpu().numpy().astype(np.float64), K, FP, drop, SEED, off)
    kw = dict(in_drop=drop, seed=SEED, row_offset=off)
    dW = ops.project_bwd(sf, dH, K, FP, **kw)
    err = rel_err(dW.cpu().numpy(), ref)
    print(f"dW ({K},{FP}) drop={drop} binary={binary}: rel err {err:.3e}")
    assert err < GTOL
    assert not dW[7].any()                                   # the empty column
    if not drop:                                             # the single entry (under dropout it may be dropped whole)
        assert dW[9].any()
    out = torch.full((F, 64), float("nan"), device=dev)      # every row is written, the empty column's too
    assert ops.project_bwd(sf, dH, K, FP, out=out, **kw) is out
    assert torch.equal(out, dW)                              # bitwise reproducible; row 7 is exactly zero
    assert not out[7].any()
    if drop:      # a device seed word, as in a captured step
        word = 77
        a = ops.project_bwd(sf, dH, K, FP, in_drop=drop, seed=SEED, row_offset=off,
                            seed_dev=torch.tensor([word], dtype=torch.int64, device=dev))
        b = ops.project_bwd(sf, dH, K, FP, in_drop=drop, seed=rng_ref.resolve_seed(SEED, word), row_offset=off)
        assert torch.equal(a, b) and not torch.equal(a, dW)


# ------------------------------------------------------------------------------------------------ 5, 6
def _problem(dev, n=300, f=70, c=3):
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(n, f, generator=g) * (torch.rand(n, f, generator=g) < 0.1)).to(dev)
    x[7] = 0                                                 # a node without words
    graphs = [synth.bernoulli_graph(n, d, seed=40 + i, device=dev) for i, d in enumerate((0.02, 0.2))]
    labels = torch.randint(0, c, (n,), generator=g).to(device=dev, dtype=torch.int32)
    mask = (torch.rand(n, generator=g) < 0.4).to(device=dev, dtype=torch.uint8)
    return x, graphs, labels, mask


def _models(count, dev, f, c, hid, heads, residual):
    from han_amd.gat import HeteGAT_multi
    first = HeteGAT_multi().build(2, f, c, hid, heads, 32, device=dev, residual=residual,
                                  generator=torch.Generator().manual_seed(9))
    with torch.no_grad():      # biases start at zero: give them values
        first.flat.add_(0.05 * torch.randn(first.flat.shape, generator=torch.Generator().manual_seed(10)).to(dev))
    out = [first]
    for _ in range(count - 1):
        m = HeteGAT_multi().build(2, f, c, hid, heads, 32, device=dev, residual=residual)
        with torch.no_grad():
            m.flat.copy_(first.flat)
        out.append(m)
    return out


def _eval_and_step(model, xs, graphs, labels, mask, c, hid, heads, residual):
    """(eval logits, training loss, gradients by name) through the public inference()."""
    n = labels.numel()
    args = (graphs, list(hid), list(heads))
    with torch.no_grad():
        logits = model.inference(xs, c, n, False, 0.0, 0.0, *args, residual=residual, mp_att_size=32)[0]
    hrng.manual_seed(123)
    model.zero_grad_flat()
    lg = model.inference(xs, c, n, True, 0.6, 0.6, *args, residual=residual, mp_att_size=32)[0][0]
    sel = mask.bool()
    loss = torch.nn.functional.cross_entropy(lg[sel], labels[sel].long())
    loss.backward()
    grads = {name: getattr(model, name).grad.detach().cpu().numpy().copy() for name, _ in model.param_shapes()}
    return logits.cpu().numpy(), float(loss), grads


@pytest.mark.parametrize("hid,heads,residual", [((8,), (8, 1), False), ((8, 8), (8, 8, 1), True), ((96,), (1, 1), False)],
                         ids=["reference-shape", "two-layers-residual", "wide-head"])
def test_dense_and_sparse_inputs_agree_through_the_model(dev, hid, heads, residual):
    x, graphs, labels, mask = _problem(dev)
    c = 3
    sf = SparseFeatures.from_dense(x)
    csr = x.to_sparse_csr()
    coo3 = x[None].to_sparse()                               # (1,N,F) COO, as the reference's batch of one
    inputs = {"dense": [x[None], x[None]], "sparse": [sf, sf], "csr": [csr, csr], "coo": [coo3, coo3],
              "mixed": [sf, x]}
    models = _models(len(inputs), dev, x.shape[1], c, hid, heads, residual)
    res = {k: _eval_and_step(m, xs, graphs, labels, mask, c, hid, heads, residual)
           for (k, xs), m in zip(inputs.items(), models)}
    lg_d, loss_d, g_d = res["dense"]
    assert np.isfinite(lg_d).all() and np.abs(lg_d).max() > 1e-3
    for k in ("sparse", "mixed"):
        lg, loss, g = res[k]
        print(f"{k}: logits {np.abs(lg - lg_d).max():.3e} loss {abs(loss - loss_d):.3e} "
              f"grads {max(rel_err(g[n], g_d[n]) for n in g):.3e}")
        assert np.abs(lg - lg_d).max() < TOL, k
        assert abs(loss - loss_d) < TOL, k
        for name in g:
            assert rel_err(g[name], g_d[name]) < GTOL, (k, name)
    for k in ("csr", "coo"):                                  # converted once, then the SparseFeatures path: same bits
        lg, loss, g = res[k]
        assert np.array_equal(lg, res["sparse"][0]) and loss == res["sparse"][1], k
        assert all(np.array_equal(g[n], res["sparse"][2][n]) for n in g), k


def test_single_head_functions_accept_sparse_seq(dev):
    from han_amd import layers
    x, graphs, _, _ = _problem(dev)
    g = torch.Generator().manual_seed(3)
    r = lambda *s: (torch.randn(*s, generator=g) * 0.3).to(dev)
    params = {"W": r(x.shape[1], 8), "a1": r(8), "a2": r(8), "b1": r(()), "b2": r(()), "c": r(8)}
    sf = SparseFeatures.from_dense(x)
    for fn, extra in ((layers.attn_head, ()), (layers.attn_head_const_1, ()), (layers.sp_attn_head, (x.shape[0],))):
        with torch.no_grad():
            want = fn(x[None], 8, graphs[0], torch.nn.functional.elu, *extra, params=params)
            for seq in (sf, x.to_sparse_csr(), x[None].to_sparse()):
                got = fn(seq, 8, graphs[0], torch.nn.functional.elu, *extra, params=params)
                assert got.shape == want.shape and float((got - want).abs().max()) < TOL, fn.__name__


def test_trainer_eager_and_captured(dev):
    """Three eager steps on sparse features land on the dense-input trainer's parameters; a captured epoch (a HIP
    graph: the entry points are capture-safe) replayed three times lands on those of the same flow launched eagerly."""
    from han_amd.trainer import HANTrainer
    x, graphs, labels, mask = _problem(dev)
    sf = SparseFeatures.from_dense(x)
    m_dense, m_sparse, m_eager, m_graph = _models(4, dev, x.shape[1], 3, (8,), (8, 1), False)
    flats = []
    for model, xs in ((m_dense, [x, x]), (m_sparse, [sf, sf])):
        tr = HANTrainer(model, xs, graphs, labels, mask, attn_drop=0.6, ffd_drop=0.6)
        hrng.manual_seed(31)
        for _ in range(3):
            tr.epoch()
        flats.append(model.flat.detach().cpu().numpy().copy())
    assert np.abs(flats[0] - _models(1, dev, x.shape[1], 3, (8,), (8, 1), False)[0].flat.cpu().numpy()).max() > 1e-3
    print(f"3 eager steps, sparse vs dense: {np.abs(flats[1] - flats[0]).max():.3e}")
    assert np.abs(flats[1] - flats[0]).max() < PTOL
    trainers = []
    for model, capture in ((m_eager, False), (m_graph, True)):
        tr = HANTrainer(model, [sf, sf], graphs, labels, mask, attn_drop=0.6, ffd_drop=0.6, use_graph=True)
        tr._capture = capture
        trainers.append(tr)
    for tr in trainers:      # one warm-up epoch, then three replayed ones: the capture's own replay and two more
        hrng.manual_seed(31)
        for _ in range(4):
            tr.epoch()
    torch.cuda.synchronize()
    assert trainers[1]._graph is not None and trainers[0]._graph is None
    a, b = (m.flat.detach().cpu().numpy() for m in (m_eager, m_graph))
    print(f"captured vs eager: {np.abs(a - b).max():.3e}")
    assert np.isfinite(b).all() and np.abs(a - b).max() < PTOL


# ------------------------------------------------------------------------------------------------ 7
def _pair_mask(seed, rows, cols, K, drop):
    """(E,K) input-dropout keep draws of the entries (rows[e], cols[e]): rng_ref.seq_mask's counters, entry by entry."""
    KQ = (K + 3) // 4
    ks = np.arange(K)[None, :]
    x, y = rng_ref.han_rand64(seed, rng_ref.STREAM_SEQ, np.asarray(rows)[:, None],
                              np.asarray(cols)[:, None].astype(np.uint64) * KQ + ks // 4)
    return (rng_ref.field(x, y, ks % 4) < rng_ref._thr(drop)).astype(np.float64)


def test_footprint_and_sampled_rows_at_size(dev):
    """65 536 x 8192 with 8 words per row: the dense fp32 image would be 2 GiB; forward + dW stay below 256 MiB."""
    n, f, K, FP, drop, off = 65536, 8192, 8, 8, 0.6, 1000
    sf = synth.bag_of_words(n, f, 8, seed=2, device=dev)
    W, a1, a2, b1, b2 = (_t(v, dev) for v in _params(K, FP, f))
    dH = torch.randn(n, 64, generator=torch.Generator().manual_seed(4)).to(dev)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    H, f1, f2 = ops.project_fwd(sf, W, a1, a2, b1, b2, in_drop=drop, fts_drop=drop, seed=SEED, row_offset=off)
    dW = ops.project_bwd(sf, dH, K, FP, in_drop=drop, seed=SEED, row_offset=off)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"peak above the starting level: {peak / 2 ** 20:.1f} MiB")
    assert peak < 256 * 2 ** 20
    t = sf.transposed()
    assert t["n_long"] > 0                                   # Zipf columns: the chunked path runs at size
    keep = rng_ref.keep_prob32(drop)
    rowptr, colidx = sf.rowptr.cpu().numpy(), sf.colidx.cpu().numpy()
    W64 = W.cpu().numpy().astype(np.float64)
    head = np.arange(64) // FP
    rows = np.concatenate([[0, n - 1], np.random.default_rng(6).choice(n, 14, replace=False)])
    Hg = H[torch.as_tensor(rows, device=dev)].cpu().numpy()
    for i, r in enumerate(rows):
        c = colidx[rowptr[r]:rowptr[r + 1]]
        m = _pair_mask(SEED, np.full(len(c), r + off), c, K, drop)[:, head]          # (E,64)
        ref = (m * W64[c]).sum(0) / keep
        assert np.abs(Hg[i] - ref).max() < TOL, r
    colptr, rowidx = t["colptr"].cpu().numpy(), t["rowidx"].cpu().numpy()
    lens = np.diff(colptr)
    order = np.argsort(lens)
    feats = np.unique(np.concatenate([order[:3], order[-5:], order[np.linspace(0, f - 1, 8).astype(int)]]))[:16]
    assert lens[feats].max() > ops.SPARSE_COL_CHUNK
    dH64 = dH.cpu().numpy().astype(np.float64)
    got = dW[torch.as_tensor(feats, device=dev)].cpu().numpy()
    worst = 0.0
    for i, ft in enumerate(feats):      # feature by feature: relative to the largest element of that feature's row
        r = rowidx[colptr[ft]:colptr[ft + 1]]
        m = _pair_mask(SEED, r + off, np.full(len(r), ft), K, drop)[:, head]
        ref = (m * dH64[r]).sum(0) / keep
        err = np.abs(got[i] - ref).max()
        assert err <= GTOL * np.abs(ref).max(), (ft, len(r), err)
        worst = max(worst, err / max(np.abs(ref).max(), 1e-30))
    print(f"dW of {len(feats)} sampled features ({lens[feats].min()} .. {lens[feats].max()} entries): rel err {worst:.3e}")
