"""The K3 backward with the row-local half of the K2 backward in its epilogue (ops.sem_attn_bwd_rows, sem_attn.hip FOLD)
against the two kernels it replaces: ops.sem_attn_bwd for dM, then ops.node_attn_bwd_rows per meta-path.

Bit-equal: dw, db, du, the g bytes, the f1 and lse words; the fourth statistics word is 0.  s and df1: the fused kernel
writes the row pass's roundings out, so they are asserted bit-equal too (the count of other values is printed first),
and, whatever that count, within the rounding-count bound of the longer of the two evaluation orders.  dc is the same
sum in another order: bounded against the float64 column sum of g."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
CASES = [(4, 16384), (4, 16387), (2, 32771), (1, 65541)]      # the smallest N * P the kernel takes; a partial last tile; a pass whose second tile lies past the end
GUARD = 3                                                       # rows of guard band on either side of the tables


def _inputs(P, N, A, dev, seed):
    from han_amd import ops
    g = torch.Generator(device="cpu").manual_seed(seed)
    rnd = lambda *sh: torch.randn(sh, generator=g)
    M = rnd(N, P, 64)
    M = torch.where(M < 0, torch.expm1(M), M)                  # ELU outputs: (-1, 0] and positive
    kind = torch.randint(0, 40, (N, P, 64), generator=g)
    M[kind == 0] = 0.0
    M[kind == 1] = -1.0                                        # an output that rounded to -1: derivative 0
    t = dict(M=M, w=rnd(64, A) * 0.1, b=rnd(A) * 0.1, u=rnd(A) * 0.1, dZ=rnd(N, 64), c=rnd(P, 64) * 0.1,
             aggp=[rnd(N, 64) for _ in range(P)], tsum=[rnd(N, 8) for _ in range(P)],
             f1=[rnd(N, 8) for _ in range(P)], lse=[rnd(N, 8) for _ in range(P)])
    t = {k: ([x.to(dev) for x in v] if isinstance(v, list) else v.to(dev)) for k, v in t.items()}
    _, t["beta"] = ops.sem_attn_fwd(t["M"], t["w"], t["b"], t["u"])
    return t


def _dc_depth(N, P):
    """Longest addition chain of the fused kernel's dc, from its geometry: grid = min(ceil(R / 64), 256) blocks of 4
    waves; a wave takes every (4 grid)-th 16-row tile, a lane adds 4 / P rows of a meta-path per tile to its register;
    the 4 lane groups of a wave are joined pairwise (2), the 4 waves in order (3); han_reduce_slabs adds at most 16 slab
    rows per thread in 4 chains (4) joined pairwise (2), then 16 partial sums in order (16)."""
    R = N * P
    grid = min(-(-R // 64), 256)
    tiles = -(-R // 16)
    per_wave = -(-tiles // (4 * grid))
    return per_wave * (4 // P) + 2 + 3 + 4 + 2 + 16


@pytest.mark.parametrize("act", ["elu", "identity"])
@pytest.mark.parametrize("A", [64, 128])
@pytest.mark.parametrize("P,N", CASES)
def test_fused_backward_matches_the_two_kernels(dev, P, N, A, act):
    from han_amd import ops
    code = ops.ACT_ELU if act == "elu" else ops.ACT_IDENTITY
    t = _inputs(P, N, A, dev, 1000 * P + A + (N % 7))
    M = t["M"]
    rb = ops.gs_row_bytes(8, 8)
    # reference: the kernels as they are
    dM, dw0, db0, du0 = ops.sem_attn_bwd(M, t["w"], t["b"], t["u"], t["beta"], t["dZ"])
    ref = [ops.node_attn_bwd_rows(dM[:, p, :], M[:, p, :], t["aggp"][p], t["tsum"][p], t["f1"][p], t["lse"][p],
                                  t["c"][p], activation=code) for p in range(P)]
    # fused, into tables with a guard band
    gs_buf = [torch.full((N + 2 * GUARD, rb), 0xA5, dtype=torch.uint8, device=dev) for _ in range(P)]
    df_buf = [torch.full((N + 2 * GUARD, 8), 123.25, device=dev) for _ in range(P)]
    dc = torch.full((P, 64), float("nan"), device=dev)
    r = ops.sem_attn_bwd_rows(M, t["w"], t["b"], t["u"], t["beta"], t["dZ"],
                              [(t["aggp"][p], t["tsum"][p], t["f1"][p], t["lse"][p]) for p in range(P)], t["c"], dc,
                              activation=code, gs_out=[b[GUARD:GUARD + N] for b in gs_buf],
                              df1_out=[b[GUARD:GUARD + N] for b in df_buf])
    assert r is not None, "the library refused an eligible shape"
    gs, df1, dw, db, du = r
    torch.cuda.synchronize()
    assert torch.equal(dw, dw0) and torch.equal(db, db0) and torch.equal(du, du0)
    depth = _dc_depth(N, P)
    n_s = n_df = 0
    for p in range(P):
        for buf in (gs_buf[p], df_buf[p]):      # nothing before the first or beyond the last row
            pat = buf[0, 0]
            assert bool((buf[:GUARD] == pat).all()) and bool((buf[GUARD + N:] == pat).all())
        g, st = ops.gs_views(gs[p])
        g0, st0 = ops.gs_views(ref[p][0])
        assert torch.equal(g.view(torch.int32), g0.view(torch.int32)), f"g bytes, meta-path {p}"
        assert torch.equal(st[..., 0].view(torch.int32), t["f1"][p].view(torch.int32))
        assert torch.equal(st[..., 1].view(torch.int32), t["lse"][p].view(torch.int32))
        assert bool((st[..., 3].view(torch.int32) == 0).all())
        assert torch.equal(st0[..., 0], st[..., 0]) and torch.equal(st0[..., 1], st[..., 1])
        # s = sum over the head's 8 columns of g (pre - c), df1 = sum g aggp - s tsum.  Both kernels are fma chains from 0
        # (4 roundings per lane, 1 for the lane pair); the longer order is the unfused one: 4 products, 3 sums (the
        # first adds to 0), 1 for the lane pair = 8, plus per term the logarithm (2) and the subtraction (1) on
        # |pre| + |c| -> 11 roundings on sum |g| (|pre| + |c|).  df1: 8 for sum g aggp, 2 for s tsum and the difference,
        # and s's bound times |tsum|.
        g64 = g.double()
        o = M[:, p, :].double()
        neg = (o <= 0) if act == "elu" else torch.zeros_like(o, dtype=torch.bool)
        da = o + 1
        pre = torch.where(neg, torch.where(da > 0, torch.log(da.clamp_min(1e-300)), torch.zeros_like(o)), o)
        t_s = (g64.abs() * (pre.abs() + t["c"][p].double().abs())).view(N, 8, 8).sum(2)
        t_d = (g64.abs() * t["aggp"][p].double().abs()).view(N, 8, 8).sum(2)
        s, s0 = st[..., 2].double(), st0[..., 2].double()
        ts_abs = t["tsum"][p].double().abs()
        bound_s = 11 * U * t_s
        bound_d = U * (8 * t_d + 2 * (t_d + s0.abs() * ts_abs)) + ts_abs * bound_s
        assert bool(((s - s0).abs() <= bound_s).all()), f"s, meta-path {p}: {float(((s - s0).abs() - bound_s).max())}"
        d, d0 = df1[p].double(), ref[p][1].double()
        assert bool(((d - d0).abs() <= bound_d).all()), f"df1, meta-path {p}: {float(((d - d0).abs() - bound_d).max())}"
        n_s += int((st[..., 2].view(torch.int32) != st0[..., 2].view(torch.int32)).sum())
        n_df += int((df1[p].view(torch.int32) != ref[p][1].view(torch.int32)).sum())
        # dc against the float64 column sum of the (bit-equal) g
        want = g64.sum(0)
        bound_c = depth * U * g64.abs().sum(0)
        err = (dc[p].double() - want).abs()
        assert bool((err <= bound_c).all()), f"dc, meta-path {p}: {float((err / bound_c).max())} of the bound (depth {depth})"
    print(f"P={P} N={N} A={A} {act}: s not bit-equal {n_s}, df1 not bit-equal {n_df} of {8 * N * P} each")
    assert n_s == 0 and n_df == 0


@pytest.mark.parametrize("why,P,N,D,A,kw", [
    ("N * P below the bf16-pipe family", 4, 16383, 64, 128, {}),
    ("P = 8", 8, 8192, 64, 128, {}),
    ("A = 256", 4, 16384, 64, 256, {}),
    ("D = 128", 4, 16384, 128, 128, {}),
    ("exact-pipe flag", 4, 16384, 64, 128, {"flags": 8}),
    ("pairs flag", 4, 16384, 64, 128, {"flags": 16}),
    ("fp32 G3 flag", 4, 16384, 64, 128, {"flags": 32}),
    ("bf16 tables", 4, 16384, 64, 128, {"table_dtype": torch.bfloat16}),
    ("4 x 16 heads", 4, 16384, 64, 128, {"K": 4, "FP": 16}),
])
def test_other_shapes_are_refused_before_any_launch(dev, why, P, N, D, A, kw):
    """The library's own check, called with real buffers: unsupported, nothing written."""
    from han_amd import _lib, ops
    import ctypes
    lib = _lib.load()
    K, FP = kw.get("K", 8), kw.get("FP", 8)
    z = lambda *sh: torch.zeros(sh, device=dev)
    M, w, b, u, beta, dZ, c = z(N, P, D), z(D, A), z(A), z(A), z(N, P), z(N, D), z(P, 64)
    tabs = [[z(N, 64) for _ in range(P)], [z(N, K) for _ in range(P)], [z(N, K) for _ in range(P)], [z(N, K) for _ in range(P)]]
    gs = [torch.full((N, 384), 7, dtype=torch.uint8, device=dev) for _ in range(P)]
    df1 = [torch.full((N, K), 7.0, device=dev) for _ in range(P)]
    outs = [torch.full(sh, 7.0, device=dev) for sh in ((D, A), (A,), (A,), (P, 64))]
    ws = torch.zeros(64 << 20, dtype=torch.uint8, device=dev)
    arr = lambda ts: (ctypes.c_void_p * P)(*[x.data_ptr() for x in ts])
    code = lib.han_sem_attn_bwd_rows(M.data_ptr(), w.data_ptr(), b.data_ptr(), u.data_ptr(), beta.data_ptr(), dZ.data_ptr(),
                                     arr(tabs[0]), arr(tabs[1]), arr(tabs[2]), arr(tabs[3]), c.data_ptr(), arr(gs), arr(df1),
                                     *[o.data_ptr() for o in outs], ws.data_ptr(), ws.numel(), N, P, D, A, K, FP,
                                     ops.DTYPE_CODE[kw.get("table_dtype", torch.float32)], 1, kw.get("flags", 0), None)
    torch.cuda.synchronize()
    assert code == _lib.E_UNSUPPORTED, why
    assert all(bool((x == 7).all()) for x in gs + df1 + outs), why


def _trainer(dev, n, fold):
    from han_amd import rng as hrng
    from han_amd import synth
    from han_amd.gat import HeteGAT_multi
    from han_amd.trainer import HANTrainer
    torch.manual_seed(0)
    hrng.manual_seed(5)
    wl = synth.planted_partition(n, 4, 4, 64, deg_in=6, deg_out=2, noise=1.0, seed=3, device=dev)
    model = HeteGAT_multi().build(4, 64, 4, (8,), (8, 1), 128, device=dev, generator=torch.Generator().manual_seed(11))
    tr = HANTrainer(model, [wl["x"]] * 4, wl["graphs"], wl["labels"], wl["train_mask"], wl["val_mask"])
    model.fold_k3 = fold
    return model, tr


def _slices(model):
    out, off = {}, 0
    for name, shp in model.param_shapes():
        n = int(np.prod(shp))
        out[name] = model.flat_grad[off:off + n].view(shp)
        off += n
    return out


def test_trainer_step_with_the_fold(dev, monkeypatch):
    """HANTrainer at N = 16 400, P = 4, degree 8, F = 64, one step, fold_k3 on against off: every gradient slice but c
    bit-equal, c within the dc bound, and the row kernel is not called."""
    from han_amd import ops
    N = 16400
    calls = {"rows": 0, "fused": []}
    rows, fused = ops.node_attn_bwd_rows, ops.sem_attn_bwd_rows

    def count_rows(*a, **k):
        calls["rows"] += 1
        return rows(*a, **k)

    def keep_fused(*a, **k):
        r = fused(*a, **k)
        calls["fused"].append(r)
        return r

    monkeypatch.setattr(ops, "node_attn_bwd_rows", count_rows)
    monkeypatch.setattr(ops, "sem_attn_bwd_rows", keep_fused)
    grads, loss = {}, {}
    for fold in (False, True):
        calls["rows"] = 0
        model, tr = _trainer(dev, N, fold)
        tl, _ = tr.train_step()
        torch.cuda.synchronize()
        loss[fold] = float(tl)
        grads[fold] = {k: v.clone() for k, v in _slices(model).items()}
        assert calls["rows"] == (0 if fold else 4), (fold, calls["rows"])
    assert loss[True] == loss[False]
    assert len(calls["fused"]) == 1 and calls["fused"][0] is not None
    for name in grads[True]:
        if name != "c":
            assert torch.equal(grads[True][name], grads[False][name]), name
    gs = calls["fused"][0][0]
    depth = _dc_depth(N, 4)
    for p in range(4):
        g64 = ops.gs_views(gs[p])[0].double()
        err = (grads[True]["c"][p].double() - g64.sum(0)).abs()
        assert bool((err <= depth * U * g64.abs().sum(0)).all()), p


def test_a_second_consumer_of_M_is_an_error(dev):
    """fold_k3 relies on semantic() being the only consumer of M: with a loss term on M as well the backward raises
    instead of dropping that term's gradient."""
    from han_amd import ops
    model, tr = _trainer(dev, 16400, True)
    with torch.enable_grad():
        M = model.node_level(tr.xs, tr.graphs, 0.6, 0.6, True, ops.ACT_ELU, graphs_t=tr.graphs_t)
        Z, _ = model.semantic(M)
        loss = Z.sum() + M.sum()
        with pytest.raises(RuntimeError, match="fold_k3"):
            loss.backward()


def test_layer_falls_back_below_the_kernel_family(dev, monkeypatch):
    """N * P < 65 536: the library reports unsupported (ops.sem_attn_bwd_rows is called and returns None) and the same
    step runs the two kernels -- the bits of fold_k3 off."""
    from han_amd import ops
    calls = {"rows": 0, "fused": []}
    rows, fused = ops.node_attn_bwd_rows, ops.sem_attn_bwd_rows

    def keep_fused(*a, **k):
        calls["fused"].append(fused(*a, **k))
        return calls["fused"][-1]

    monkeypatch.setattr(ops, "sem_attn_bwd_rows", keep_fused)

    def count_rows(*a, **k):
        calls["rows"] += 1
        return rows(*a, **k)

    monkeypatch.setattr(ops, "node_attn_bwd_rows", count_rows)
    flats = []
    for fold in (False, True):
        calls["rows"] = 0
        model, tr = _trainer(dev, 2000, fold)
        tr.train_step()
        torch.cuda.synchronize()
        flats.append(model.flat_grad.clone())
        assert calls["rows"] == 4
    assert calls["fused"] == [None]
    assert torch.equal(flats[0], flats[1])
