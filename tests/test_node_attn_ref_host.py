"""CPU checks of tests/node_attn_ref.py, the float64 reference and the error bounds of the K2 GPU tests:
the reference against the oracle (dense -1e9 mask softmax, autograd for the backward formulas), the bounds against planted
errors (they must exclude them) and against an fp32 evaluation in another summation order (they must admit it), and the
case generators against CSRGraph.row_bins / row_split and the grid arithmetic."""
import numpy as np
import pytest
import torch

from oracle import han_oracle_torch as OT
from tests import node_attn_ref as R
from tests import rng_ref

CD, FD, SEED = 0.6, 0.5, 11


def _small_graph(n, seed=0, max_len=None):
    """n rows against an n-row table, lengths 0 .. max_len mixed, columns distinct within a row, first and last row
    non-empty."""
    rng = np.random.default_rng([n, seed])
    max_len = min(n, 40) if max_len is None else max_len
    lens = rng.integers(0, max_len + 1, size=n)
    lens[0], lens[-1] = max(lens[0], 2), max(lens[-1], 3)
    lens[n // 2] = 0
    return R.graph_from_lengths(lens, n, stride=1 if n < 14 else 13)


def _chain(n, K, FP, *, bf16=False, val=False, res=False, elu=True, cd=CD, fd=FD, seed=0, plant_f=(), plant_r=()):
    """The whole reference chain in float64 on an n-row graph: forward (training), row-local backward from the
    reference's own outputs, transposed-graph backward from the reference's own gs table, score gradients."""
    rowptr, colidx = _small_graph(n, seed)
    d = R.fwd_inputs(K, FP, bf16, n, n, "plain", fd, seed)
    rng = np.random.default_rng([n, K, seed, 5])
    a1 = (rng.standard_normal((K, FP)) * 0.3).astype(np.float32)
    b1 = (rng.standard_normal(K) * 0.1).astype(np.float32)
    dOut = rng.standard_normal((n, 64)).astype(np.float32)
    values = R.edge_values(len(colidx), seed) if val else None
    H64 = R.up(d["H"])
    f1 = (H64.reshape(n, K, FP) * R.up(a1)).sum(-1) + R.up(b1)
    f2 = (H64.reshape(n, K, FP) * R.up(d["a2"])).sum(-1) + R.up(d["b2"])
    resv = d["res"] if res else None
    fw = R.fwd_ref(rowptr, colidx, d["H"], f1, d["a2"], d["b2"], d["c"], bf16=bf16, values=values, train=True,
                   coef_drop=cd, fts_drop=fd, seed=SEED, res=resv, elu=elu, want_coef=True, plant=plant_f)
    br = R.bwd_rows_ref(R.up(dOut), fw.out, fw.aggp, fw.tsum, f1, fw.lse, d["c"], K, FP, res=resv, elu=elu, bf16=bf16,
                        plant=plant_r)
    stats = np.stack([f1, fw.lse, br.s, np.zeros_like(br.s)], -1)
    tr = R.transpose(rowptr, colidx, n, values)
    bc = R.bwd_cols_ref(tr[0], tr[1], br.gs, stats, d["H"], f2, br.df1, a1, d["a2"], bf16=bf16,
                        values=tr[2] if val else None, coef_drop=cd, fts_drop=fd, seed=SEED)
    sc = R.score_ref(H64, br.df1, bc.df2, K, FP, R.depth_rows(n))
    return dict(rowptr=rowptr, colidx=colidx, d=d, a1=a1, b1=b1, dOut=dOut, values=values, f1=f1, f2=f2, fw=fw, br=br,
                bc=bc, sc=sc, tr=tr, stats=stats)


# ------------------------------------------------------------------------------------------------ against the oracle
@pytest.mark.parametrize("n,K,FP,val,res,elu", [(7, 8, 8, False, False, True), (16, 8, 8, False, True, True),
                                                (33, 4, 16, False, False, False), (64, 1, 64, False, True, True),
                                                (24, 16, 4, True, False, True), (40, 2, 32, True, True, False)])
def test_reference_against_the_oracle(monkeypatch, n, K, FP, val, res, elu):
    monkeypatch.setattr(OT, "LEAKY_ALPHA", R.SLOPE)      # the kernels take the slope as a C float: 0.2f, not 0.2
    ch = _chain(n, K, FP, val=val, res=res, elu=elu)
    d, rowptr, colidx = ch["d"], ch["rowptr"], ch["colidx"]
    tt = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))
    x = tt(R.up(d["H"])).requires_grad_(True)
    par = {k: tt(R.up(v)).requires_grad_(True) for k, v in (("a1", ch["a1"]), ("b1", ch["b1"]), ("a2", d["a2"]),
                                                            ("b2", d["b2"]), ("c", d["c"]))}
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    coef = rng_ref.coef_draws(SEED, rows, colidx, K, CD)                      # (E, K)
    fts = R.keep_bits(d["H"], False)
    keep_c, keep_f = 1.0 / R.inv_keep(CD), 1.0 / R.inv_keep(FD)
    eye = torch.eye(64, dtype=torch.float64)
    if val:
        out = OT.node_attention_csr(x, torch.tensor(rowptr), torch.tensor(colidx.astype(np.int64)), eye,
                                    par["a1"], par["b1"], par["a2"], par["b2"], par["c"], keep_in=keep_f, keep_coef=keep_c,
                                    masks={"coef": tt(coef), "fts": tt(fts)}, adj_vals=tt(ch["values"]))
    else:
        bias = np.full((n, n), -1e9)
        bias[rows, colidx] = 0.0
        cm = np.zeros((K, n, n))
        cm[:, rows, colidx] = coef.T
        out = OT.node_attention_dense(x, tt(bias), eye, par["a1"], par["b1"], par["a2"], par["b2"], par["c"],
                                      keep_in=keep_f, keep_coef=keep_c, masks={"coef": tt(cm), "fts": tt(fts)})
    # the oracle has no residual input and always applies ELU: the reference is taken without the one and through the other
    fw0 = R.fwd_ref(rowptr, colidx, d["H"], ch["f1"], d["a2"], d["b2"], d["c"], values=ch["values"], train=True,
                    coef_drop=CD, fts_drop=FD, seed=SEED, elu=False)
    if res:
        assert np.abs(ch["fw"].pre - fw0.pre - R.up(d["res"])).max() < 1e-12
    if not elu:
        assert np.array_equal(ch["fw"].out, ch["fw"].pre)
    ref_elu = np.where(fw0.pre > 0, fw0.pre, np.expm1(np.minimum(fw0.pre, 0)))
    # (the dense form gives an empty row the uniform average over ALL columns; the CSR kernels give act(c + res))
    live = np.ones(n, bool) if val else np.diff(rowptr) > 0
    got = out.detach().numpy()
    assert np.abs(got[live] - ref_elu[live]).max() < 1e-11
    if res:
        return       # the backward of a residual case is the same formulas from another `out`: covered without it
    # backward: g of the chain is dOut act'(pre); the oracle differentiates ELU, so it is fed dOut / elu' for identity
    da = np.where(fw0.pre > 0, 1.0, np.exp(np.minimum(fw0.pre, 0)))
    dO = R.up(ch["dOut"]) * live[:, None]
    (out * tt(dO * (1.0 if elu else 1.0 / da))).sum().backward()
    fw = ch["fw"]
    br = R.bwd_rows_ref(dO, fw.out, fw.aggp, fw.tsum, ch["f1"], fw.lse, d["c"], K, FP, elu=elu)
    stats = np.stack([ch["f1"], fw.lse, br.s, np.zeros_like(br.s)], -1)
    tr = ch["tr"]
    bc = R.bwd_cols_ref(tr[0], tr[1], br.gs, stats, d["H"], ch["f2"], br.df1, ch["a1"], d["a2"],
                        values=tr[2] if val else None, coef_drop=CD, fts_drop=FD, seed=SEED)
    sc = R.score_ref(R.up(d["H"]), br.df1, bc.df2, K, FP, 1)
    tol = lambda a: 1e-10 * max(1.0, float(np.abs(a).max()))
    assert np.abs(x.grad.numpy() - bc.dH).max() < tol(bc.dH)
    assert np.abs(par["c"].grad.numpy() - br.dc).max() < tol(br.dc)
    for name in ("a1", "a2", "b1", "b2"):
        assert np.abs(par[name].grad.numpy() - getattr(sc, "d" + name)).max() < tol(getattr(sc, "d" + name)), name


def test_reference_forward_against_the_numpy_oracle():
    """oracle/han_oracle.py: head by head, dense -1e9 mask, eval."""
    from oracle import han_oracle as O
    n, K, FP = 21, 8, 8
    rowptr, colidx = _small_graph(n, 3)
    d = R.fwd_inputs(K, FP, False, n, n, "plain", 0.0, 3)
    H64 = R.up(d["H"]).reshape(n, K, FP)
    f1 = (H64 * R.up(d["a2"])).sum(-1) * 0.5
    fw = R.fwd_ref(rowptr, colidx, d["H"], f1, d["a2"], d["b2"], d["c"])
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    bias = np.full((n, n), -1e9)
    bias[rows, colidx] = 0.0
    f2 = (H64 * R.up(d["a2"])).sum(-1) + R.up(d["b2"])
    ne = np.diff(rowptr) > 0
    for k in range(K):
        coefs = O.softmax(O.leaky_relu(f1[:, k, None] + f2[None, :, k], R.SLOPE) + bias)
        want = O.elu(coefs @ H64[:, k] + R.up(d["c"])[k * FP:(k + 1) * FP])
        assert np.abs(want[ne] - fw.out[ne, k * FP:(k + 1) * FP]).max() < 1e-12


# ------------------------------------------------------------------------------------------------ planted errors
def _exceeds(variant, ref, e, min_share=0.0):
    """The planted error lies outside the bound: in every row it changes, and on at least 97 % of the elements it changes
    by more than float64 noise (a head whose scores all have one sign keeps tsum = 1 or slope whatever entries it holds;
    an element that the error itself moves by less than e -- a term that happens to cancel -- no bound can see).  It
    must change at least min_share of the elements."""
    variant, ref = np.asarray(variant, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    d = np.abs(variant - ref)
    changed = d > 1e-13 * (1.0 + np.abs(ref))
    assert changed.any() and changed.sum() >= min_share * changed.size, changed.mean()
    out = (d > e) & changed
    assert out.sum() >= 0.97 * changed.sum(), (int(out.sum()), int(changed.sum()))
    rows = changed.reshape(changed.shape[0], -1) if changed.ndim > 1 else changed[None]
    assert (out.reshape(rows.shape).any(1) == rows.any(1)).all()


@pytest.mark.parametrize("K,FP", [(8, 8), (2, 32)])
def test_bounds_exclude_planted_errors_forward(K, FP):
    n = 48
    ch = _chain(n, K, FP, res=True)
    fw, rowptr, colidx, d = ch["fw"], ch["rowptr"], ch["colidx"], ch["d"]
    kw = dict(train=True, coef_drop=CD, fts_drop=FD, seed=SEED, res=d["res"], want_coef=True)
    deg = np.diff(rowptr)
    # one dropped entry in one row (the longest: the smallest relative change)
    i = int(deg.argmax())
    keep = np.ones(len(colidx), bool)
    keep[rowptr[i] + deg[i] // 2] = False
    rp2 = rowptr.copy()
    rp2[i + 1:] -= 1
    v = R.fwd_ref(rp2, colidx[keep], d["H"], ch["f1"], d["a2"], d["b2"], d["c"], **kw)
    for name in ("out", "lse", "aggp", "tsum"):
        _exceeds(getattr(v, name)[i], getattr(fw, name)[i], getattr(fw, "e_" + name)[i], 0.9 if name != "tsum" else 0.0)
    # a row shifted by one; two heads swapped
    for name in ("out", "lse", "aggp", "tsum"):
        x, e = getattr(fw, name), getattr(fw, "e_" + name)
        _exceeds(np.roll(x, 1, axis=0), x, e, 0.7)
        xs = x.reshape(n, K, -1).copy()
        xs[:, [0, 1]] = xs[:, [1, 0]]
        _exceeds(xs.reshape(x.shape), x, e, 0.7 * 2 / K)
    # the keep bit ignored, the mask drawn with (src, dst) swapped, 1 / keep applied twice
    for plant, share in (("ignore_keep", 0.5), ("swap_mask", 0.5), ("keep_twice", 0.8)):
        v = R.fwd_ref(rowptr, colidx, d["H"], ch["f1"], d["a2"], d["b2"], d["c"], plant=(plant,), **kw)
        _exceeds(v.out, fw.out, fw.e_out, share)
        _exceeds(v.aggp, fw.aggp, fw.e_aggp, share)
        if plant == "swap_mask":
            _exceeds(v.coef, fw.coef, fw.e_coef, 0.3)


@pytest.mark.parametrize("K,FP", [(8, 8), (1, 64)])
def test_bounds_exclude_planted_errors_backward(K, FP):
    n = 48
    ch = _chain(n, K, FP, bf16=True)
    br, bc, fw, d = ch["br"], ch["bc"], ch["fw"], ch["d"]
    args = (R.up(ch["dOut"]), fw.out, fw.aggp, fw.tsum, ch["f1"], fw.lse, d["c"], K, FP)
    v = R.bwd_rows_ref(*args, bf16=True, plant=("s_with_c",))
    _exceeds(v.s, br.s, br.e_s, 0.9)
    _exceeds(v.df1, br.df1, br.e_df1, 0.9)
    v = R.bwd_rows_ref(*args, bf16=True, plant=("unrounded_g",))
    _exceeds(v.df1, br.df1, br.e_df1, 0.9)
    # a g stored one bf16 step off lies outside [g_lo, g_hi]
    step = np.abs(br.gs) * 2.0 ** -7
    nz = br.gs != 0
    assert ((br.gs + step > br.g_hi) & (br.gs - step < br.g_lo))[nz].all()
    assert ((br.g_lo <= br.gs) & (br.gs <= br.g_hi)).all()
    # the transposed-graph pass: a dropped entry, a shifted row, two heads swapped, the keep bit ignored, a wrong key
    colptr, rowidx = ch["tr"][0], ch["tr"][1]
    deg = np.diff(colptr)
    j = int(deg.argmax())
    keep = np.ones(len(rowidx), bool)
    keep[colptr[j] + deg[j] // 2] = False
    cp2 = colptr.copy()
    cp2[j + 1:] -= 1
    kw = dict(bf16=True, coef_drop=CD, fts_drop=FD, seed=SEED)
    v = R.bwd_cols_ref(cp2, rowidx[keep], br.gs, ch["stats"], d["H"], ch["f2"], br.df1, ch["a1"], d["a2"], **kw)
    _exceeds(v.df2[j], bc.df2[j], bc.e_df2[j], 0.9)
    _exceeds(v.dH[j], bc.dH[j], bc.e_dH[j], 0.4)
    for name in ("dH", "df2"):
        x, e = getattr(bc, name), getattr(bc, "e_" + name)
        _exceeds(np.roll(x, 1, axis=0), x, e, 0.7)
        if K > 1:
            xs = x.reshape(n, K, -1).copy()
            xs[:, [0, 1]] = xs[:, [1, 0]]
            _exceeds(xs.reshape(x.shape), x, e, 0.7 * 2 / K)
    Hc = R.stamp_keep_bits(d["H"], True, np.ones((n, 64), dtype=np.uint32))      # every keep bit set: the bit ignored
    v = R.bwd_cols_ref(colptr, rowidx, br.gs, ch["stats"], Hc, ch["f2"], br.df1, ch["a1"], d["a2"], **kw)
    _exceeds(v.dH, bc.dH, bc.e_dH, 0.3)
    v = R.bwd_cols_ref(colptr, rowidx, br.gs, ch["stats"], d["H"], ch["f2"], br.df1, ch["a1"], d["a2"], src_offset=1, **kw)
    _exceeds(v.df2, bc.df2, bc.e_df2, 0.5)
    # score gradients: a dropped row
    sc = ch["sc"]
    df1z = br.df1.copy()
    df1z[n // 3] = 0
    v = R.score_ref(R.up(d["H"]), df1z, bc.df2, K, FP, R.depth_rows(n))
    _exceeds(v.da1, sc.da1, sc.e_da1, 0.8)
    _exceeds(v.db1, sc.db1, sc.e_db1, 0.8)


# ------------------------------------------------------------------------------------------------ a correct fp32 kernel
def _f32_forward(ch, K, FP, bf16, val):
    """The same formulas in fp32, two-pass softmax, every sum taken sequentially from the LAST entry to the first."""
    f = np.float32
    rowptr, colidx, d = ch["rowptr"], ch["colidx"], ch["d"]
    n = len(rowptr) - 1
    H = d["H"].reshape(n, K, FP)
    keep = R.keep_bits(d["H"], bf16).reshape(n, K, FP).astype(f)
    ikc, ikf = f(R.inv_keep(CD)), f(R.inv_keep(FD))
    a2, b2, c = d["a2"], d["b2"], d["c"]
    f1 = ch["f1"].astype(f)
    slope = f(R.SLOPE)
    rsum = lambda a: np.cumsum(a[::-1], axis=0, dtype=f)[-1]
    hsum = lambda a: np.cumsum(a[..., ::-1], axis=-1, dtype=f)[..., -1]
    out, aggp = np.zeros((n, K, FP), f), np.zeros((n, K, FP), f)
    lse, tsum = np.full((n, K), f(R.NEG_BIG)), np.zeros((n, K), f)
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    draws = rng_ref.coef_draws(SEED, rows, colidx, K, CD).astype(f)
    vals = ch["values"] if val else np.ones(len(colidx), f)
    for i in range(n):
        s, e = rowptr[i], rowptr[i + 1]
        agg = np.zeros((K, FP), f)
        if e > s:
            j = colidx[s:e]
            w = vals[s:e, None]
            f2 = hsum(H[j] * a2) + b2
            x = (f1[i] + f2) * w
            sg = np.where(x > 0, f(1), slope) * w
            ee = np.maximum(x, slope * x)
            m = ee.max(0)
            p = np.exp(ee - m)
            l = rsum(p)
            lse[i] = m + np.log(l)
            tsum[i] = rsum(p * sg) / l
            hd = H[j] * keep[j]
            pd = (p * draws[s:e])[:, :, None]
            scale = (f(1) / l * ikc * ikf)[:, None]
            agg = rsum(pd * hd) * scale
            aggp[i] = rsum(pd * sg[:, :, None] * hd) * scale
        pre = agg + c.reshape(K, FP)
        out[i] = np.where(pre > 0, pre, np.exp(np.minimum(pre, f(0))) - f(1))
    return out.reshape(n, 64), lse, aggp.reshape(n, 64), tsum


@pytest.mark.parametrize("K,FP,bf16,val", [(8, 8, False, False), (8, 8, True, True), (1, 64, False, True),
                                           (16, 4, True, False), (4, 16, False, False), (2, 32, True, True)])
def test_bounds_admit_an_fp32_evaluation_in_another_order(K, FP, bf16, val):
    f = np.float32
    n = 64
    ch = _chain(n, K, FP, bf16=bf16, val=val)
    fw, d = ch["fw"], ch["d"]
    out, lse, aggp, tsum = _f32_forward(ch, K, FP, bf16, val)
    ratios = R.fwd_ratios(fw, out, (lse, aggp, tsum))
    assert all(0 < v <= 1 for v in ratios.values()), ratios
    # the backward halves in fp32 from the fp32 forward's own state
    dOut = ch["dOut"]
    neg = out <= 0
    da = np.where(neg, out + f(1), f(1)).astype(f)
    pre = np.where(neg, np.log(np.where(da > 0, da, f(1))), out).astype(f)
    g = (dOut * da).astype(f)
    gst = R.bf16_round(g).astype(f) if bf16 else g
    hsum = lambda a: np.cumsum(a.reshape(n, K, FP)[..., ::-1], axis=-1, dtype=f)[..., -1]
    s = hsum(gst * (pre - d["c"]))
    df1 = (hsum(gst * aggp) - s * tsum).astype(f)
    dc = np.cumsum(g[::-1], axis=0, dtype=f)[-1]
    br = R.bwd_rows_ref(dOut, out, aggp, tsum, ch["f1"].astype(f), lse, d["c"], K, FP, bf16=bf16, g_stored=gst)
    assert ((br.g_lo <= gst) & (gst <= br.g_hi)).all()
    rr = dict(s=R.ratio(s, br.s, br.e_s), df1=R.ratio(df1, br.df1, br.e_df1), dc=R.ratio(dc, br.dc, br.e_dc))
    assert all(0 < v <= 1 for v in rr.values()), rr
    # transposed-graph pass in fp32, last entry first
    colptr, rowidx = ch["tr"][0], ch["tr"][1]
    tv = ch["tr"][2] if val else np.ones(len(rowidx), f)
    stats = np.stack([ch["f1"].astype(f), lse, s, np.zeros_like(s)], -1).astype(f)
    f2 = ch["f2"].astype(f)
    H = d["H"].reshape(n, K, FP)
    mk = (R.keep_bits(d["H"], bf16).reshape(n, K, FP) * R.inv_keep(FD)).astype(f)
    hd = (H * mk).astype(f)
    src = np.repeat(np.arange(n), np.diff(colptr))
    am = (rng_ref.coef_draws(SEED, rowidx, src, K, CD) * R.inv_keep(CD)).astype(f)
    dH, df2 = np.zeros((n, K, FP), f), np.zeros((n, K), f)
    slope = f(R.SLOPE)
    for j in range(n):
        a, b = colptr[j], colptr[j + 1]
        acc = np.zeros((K, FP), f)
        if b > a:
            i = rowidx[a:b]
            w = tv[a:b, None]
            x = (stats[i, :, 0] + f2[j]) * w
            sg = np.where(x > 0, f(1), slope) * w
            alpha = np.exp(np.maximum(x, slope * x) - stats[i, :, 1])
            gk = gst.reshape(n, K, FP)[i]
            dot = np.cumsum((gk * hd[j])[..., ::-1], axis=-1, dtype=f)[..., -1]
            df2[j] = np.cumsum((alpha * sg * (am[a:b] * dot - stats[i, :, 2]))[::-1], axis=0, dtype=f)[-1]
            acc = np.cumsum(((alpha * am[a:b])[:, :, None] * gk)[::-1], axis=0, dtype=f)[-1]
        dH[j] = acc * mk[j] + df1[j][:, None] * ch["a1"] + df2[j][:, None] * d["a2"]
    bc = R.bwd_cols_ref(colptr, rowidx, gst, stats, d["H"], f2, df1, ch["a1"], d["a2"], bf16=bf16,
                        values=tv if val else None, coef_drop=CD, fts_drop=FD, seed=SEED)
    rc = dict(dH=R.ratio(dH.reshape(n, 64), bc.dH, bc.e_dH), df2=R.ratio(df2, bc.df2, bc.e_df2))
    assert all(0 < v <= 1 for v in rc.values()), rc
    sums = (np.einsum("jk,jkf->kf", df1, H).astype(f), np.einsum("jk,jkf->kf", df2, H).astype(f), df1.sum(0), df2.sum(0))
    sr = R.score_ratios(R.score_ref(d["H"], df1, df2, K, FP, R.depth_rows(n)), sums)
    assert all(v <= 1 for v in sr.values()), sr


# ------------------------------------------------------------------------------------------------ case generators
def _csr(rowptr, colidx, nt):
    from han_amd.graph import CSRGraph
    return CSRGraph(torch.tensor(rowptr), torch.tensor(colidx), n_cols=nt)


def test_edge_graph_is_what_the_gpu_tests_claim():
    rowptr, colidx = R.edge_graph()
    deg = np.diff(rowptr)
    assert set(R.EDGE_LENGTHS) | set(R.EDGE_LONG) == set(deg.tolist())
    assert all((deg == n).sum() == 1 for n in R.EDGE_LONG) and 380 <= len(deg) <= 420
    assert deg[0] > 0 and deg[-1] > 0 and colidx.max() < R.EDGE_NT
    for i in range(len(deg)):
        row = colidx[rowptr[i]:rowptr[i + 1]]
        assert len(set(row.tolist())) == len(row)
    assert R.SPLIT_DEG in deg and R.SPLIT_DEG - 1 in deg and R.SPLIT_DEG + 1 in deg


@pytest.mark.parametrize("split", [(R.SPLIT_DEG, R.SPLIT_CHUNK), (48, 16)])
def test_row_forms_and_grids_mirror_the_host_dispatch(split):
    from han_amd import ops
    assert (ops.SHORT_DEG, ops.SPLIT_DEG, ops.SPLIT_CHUNK) == (R.SHORT_DEG, R.SPLIT_DEG, R.SPLIT_CHUNK)
    assert abs(ops.LEAKY_SLOPE - 0.2) < 1e-12 and ops.GS_Z_ALL_ZERO == R.GS_Z_ALL_ZERO
    rowptr, colidx = R.edge_graph()
    for rp, ci, nt in ((rowptr, colidx, R.EDGE_NT), R.transpose(rowptr, colidx, R.EDGE_NT) + (len(rowptr) - 1,)):
        g = _csr(rp, ci, nt)
        deg = np.diff(rp)
        forms = R.row_forms(deg, True, split[0])
        rb = g.row_bins(R.SHORT_DEG, split[0])
        sp = g.row_split(*split)
        assert rb["n_short"] == (forms == R.SHORT).sum() and rb["n_mid"] == (forms == R.WAVE).sum()
        if rb["short_rows"] is not None:
            assert (np.sort(rb["short_rows"].numpy()) == np.nonzero(forms == R.SHORT)[0]).all()
        longs = np.nonzero(forms == R.CHUNK)[0]
        if len(longs):
            assert (sp["long_rows"].numpy() == longs).all()
            assert sp["n_chunks"] == sum(-(-int(n) // split[1]) for n in deg[longs])
            assert int((sp["chunk_end"] - sp["chunk_start"]).max()) <= split[1]
            assert R.grid_passes(deg, True, *split)["chunk"][0] == sp["n_chunks"]
        else:
            assert sp is None
    if split[0] == 48:
        assert -(-2500 // 16) > 64          # the finish kernel's loop over 64 chunks turns
    assert R.attn_grid(1) == 1 and R.attn_grid(4 * 8192) == 8192 and R.attn_grid(10 ** 9) == 8192


def test_loop_graphs_pass_every_grid_loop_twice():
    for kind, launch, units in (("wave", "wave", 2 * 32768 + 5), ("short", "short", 2 * 32768 + 2), ("chunk", "chunk", 2 * 32768 + 5)):
        rowptr, colidx = R.loop_graph(kind)
        deg = np.diff(rowptr)
        split = R.LOOP_SPLIT if kind == "chunk" else (R.SPLIT_DEG, R.SPLIT_CHUNK)
        passes = R.grid_passes(deg, True, *split)
        assert list(passes) == [launch] and passes[launch] == (units, R.GRID_CAP, 3)
        assert colidx.max() < R.LOOP_NT and deg.max() <= 48
        if kind == "short":
            assert len(deg) == 2 * 131072 + 7 and deg.min() == 1 and deg.max() == 15
        if kind == "wave":
            assert deg.min() == 16 and deg.max() == 24
        if kind == "chunk":
            g = _csr(rowptr, colidx, R.LOOP_NT)
            assert g.row_split(*R.LOOP_SPLIT)["n_chunks"] == units and (deg > 16).all()
    grid = min(-(-R.LOOP_ROWS // 16), R.REDUCE_BLOCKS)
    assert grid == R.REDUCE_BLOCKS and -(-R.LOOP_ROWS // (16 * grid)) == 3 and R.LOOP_ROWS == 2 * 16 * grid + 5


def test_lean_graphs_are_what_the_lean_dispatch_takes():
    from han_amd import ops
    rowptr, colidx = R.lean_graph()
    g = _csr(rowptr, colidx, R.LEAN_NT)
    H = torch.zeros((R.LEAN_NT, 64))
    assert ops._use_lean(g, H) and g.nnz < ops.DENSE_MIN_DENSITY * g.n_rows * g.n_cols
    assert ops._use_lean(_csr(*R.graph_from_lengths(np.full(R.LEAN_LOOP_ROWS, 64), R.LOOP_NT), R.LOOP_NT), torch.zeros((R.LOOP_NT, 64)))
    deg = np.diff(rowptr)
    assert {0, 1, 15, 16, 17, 63, 64, 65, 333} <= set(deg.tolist()) and not g.nnz < R.LOW_DEGREE * g.n_rows
    pick = R.lean_loop_sample()
    per = 4 * R.GRID_CAP
    assert 4096 <= len(pick) <= 4096 + 5 * 256 + 5 and -(-R.LEAN_LOOP_ROWS // per) == 3
    assert all({lo, lo + 255, min(lo + per, R.LEAN_LOOP_ROWS) - 1} <= set(pick.tolist()) for lo in range(0, R.LEAN_LOOP_ROWS, per) if lo + 255 < R.LEAN_LOOP_ROWS)
    # the lean paths cover a direct count of both kernels' loops: adds of a lane group, steps of 16 edges, folds
    for n in (0, 1, 15, 16, 17, 63, 64, 65, 200, 333):
        steps = sum(-(-min(64, n - b) // 16) for b in range(0, n, 64))
        assert R._p_wave(np.int64(n)) + R.FOLD >= -(-n // 4) + 3 * steps + 3 * R.FOLD - R.FOLD
        assert R._p_wave(np.int64(n)) + R.FOLD >= -(-n // 8) + 3 * steps + 3 * R.FOLD


@pytest.mark.parametrize("n,nt", [(130, 130), (1000, 777), (3000, 4057), (64, 16384)])
def test_dense_graphs_and_the_segment_split(n, nt):
    """dense_split against the workspace size the library asks for: header + S x rows x row width floats."""
    from han_amd import _lib, ops
    lib = _lib.load()
    tiles, S = R.dense_split(n, nt)
    assert tiles == -(-nt // 32) and 1 <= S <= tiles
    for train, rw in ((0, 72), (1, 144)):
        assert lib.han_node_attn_dense_workspace(n, nt, train) == 4 * (32 + 16 * 32) + 4 * S * n * rw
    if n <= 1000:
        rowptr, colidx = R.dense_graph(n, nt)
        deg = np.diff(rowptr)
        assert rowptr[-1] >= ops.DENSE_MIN_DENSITY * n * nt and deg.min() == 0 and deg.max() == nt
        assert ops._use_lean(_csr(rowptr, colidx, nt), torch.zeros((nt, 64)))
        assert all(len(set(colidx[rowptr[i]:rowptr[i + 1]].tolist())) == deg[i] for i in range(0, n, 7))
        d = R.fwd_inputs(8, 8, False, n, nt, "plain", 0.5)
        assert R.dense_applies(d["f2"]) and not R.dense_applies(R.fwd_inputs(8, 8, False, n, nt, "wide", 0.5)["f2"])
        assert R.dense_applies(R.bwd_cols_inputs(8, 8, False, n, nt, 0.5)["f2"])


def test_paths_cover_the_kernel_loops():
    """The path lengths against a direct count of the loops of node_attn_fwd_kernel (RPW = 1, U = 4, SPLIT)."""
    for n in list(range(0, 200)) + [1023, 1024, 2500]:
        steps = 0
        for base in range(0, n, 64):
            cnt = min(64, n - base)
            it = 0
            while (it + 4) * 4 <= cnt:
                it += 4
                steps += 1
            while it * 4 < cnt:
                it += 1
                steps += 1
        assert R._steps_wave(np.int64(n)) == steps
        assert R._p_wave(np.int64(n)) == -(-n // 4) + 3 * steps + 2 * R.FOLD


def test_cells_name_every_gather_instance_once():
    assert len(set(R.CELLS)) == len(R.CELLS)
    for K, FP in R.HEADS:
        for bf in (0, 1):
            assert f"bwd_rows<FP={FP},BF={bf}>" in R.CELLS and f"score_param<FP={FP},BF={bf}>" in R.CELLS
        assert f"fwd_finish<FP={FP},TRAIN=1>" in R.CELLS and f"coef<K={K}>" in R.CELLS
    assert "fwd<FP=8,TRAIN=1,RPW=1,U=4,BF=0,VAL=0,FAST=1,SPLIT=1,DD=1>" in R.CELLS
    assert not any(c.startswith("bwd_cols") and "BF=1" in c and "MODE=0" not in c and "MODE=4" not in c for c in R.CELLS)


@pytest.mark.parametrize("K,FP", R.HEADS)
def test_reference_alone_stays_inside_the_exclusion_cap(K, FP):
    """No generator leaves more than 1 % of a tensor to an undecided sign or a flushed alpha."""
    rowptr, colidx = R.edge_graph()
    n = len(rowptr) - 1
    for kind in ("plain", "wide"):
        d = R.fwd_inputs(K, FP, False, n, R.EDGE_NT, kind, 0.5)
        fw = R.fwd_ref(rowptr, colidx, d["H"], d["f1"], d["a2"], d["b2"], d["c"], train=True, coef_drop=CD, fts_drop=0.5)
        assert fw.undecided <= 0.01 * len(colidx) * K
        assert np.isfinite(fw.e_out).all() and np.isfinite(fw.e_aggp).all()
    colptr, rowidx = R.transpose(rowptr, colidx, R.EDGE_NT)
    b = R.bwd_cols_inputs(K, FP, False, R.EDGE_NT, n, 0.5)
    bc = R.bwd_cols_ref(colptr, rowidx, b["g"], b["stats"], b["H"], b["f2"], b["df1"], b["a1"], b["a2"], coef_drop=CD,
                        fts_drop=0.5)
    assert bc.flushed <= 0.01 * bc.entries and np.isfinite(bc.e_dH).all()
