"""Checks of tests/sem_attn_ref.py that need no GPU: the float64 reference against the oracle and float64 autograd, the
bounds against a plain fp32 restatement (not too tight) and against single-node / single-row mistakes (not too loose),
the preconditions of the shared cases, and the mirrored dispatch constants against han_amd/csrc/sem_attn.hip."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import han_oracle as ho
from oracle import han_oracle_torch as ht
from tests import sem_attn_ref as R

SHAPES = sorted({(c.P, c.D, c.A) for c in R.CELLS})
P_CLASSES = [(1, 64, 64), (4, 64, 128), (16, 64, 128), (3, 64, 64), (33, 64, 64), (64, 64, 128), (5, 128, 192),
             (3, 192, 384)]
_HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "han_amd", "csrc", "sem_attn.hip")


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("P,D,A", P_CLASSES)
def test_reference_matches_oracle_and_autograd(P, D, A):
    case, ref = R.small_ref("dense", 37, P, D, A)
    M, w, b, u, dZ = (R.up(case[k]) for k in ("M", "w", "b", "u", "dZ"))
    Zo, bo = ho.simple_att_layer(M, w, b, u, return_alphas=True)
    assert np.abs(ref.Z - Zo).max() <= 1e-12 and np.abs(ref.beta - bo).max() <= 1e-12
    tM, tw, tb, tu = (torch.tensor(x, requires_grad=True) for x in (M, w, b, u))
    Zt, _ = ht.semantic_attention(tM, tw, tb, tu)
    (Zt * torch.tensor(dZ)).sum().backward()
    for name, got, want in (("dM", ref.dM, tM.grad), ("dW", ref.dW, tw.grad), ("db", ref.db, tb.grad),
                            ("du", ref.du, tu.grad)):
        want = want.numpy()
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), name


# ------------------------------------------------------------------------------------------------ not too tight
def restate(case, beta_in=None):
    """The same formulas in fp32 (torch, CPU), tanh written as the kernel writes it."""
    M, w, b, u, dZ = (torch.from_numpy(np.ascontiguousarray(case[k])) for k in ("M", "w", "b", "u", "dZ"))
    N, P, D = M.shape
    pre = M @ w + b
    v = 1.0 - 2.0 / (1.0 + torch.exp(2.0 * pre))
    s = v @ u
    ex = torch.exp(s - s.max(1, keepdim=True).values)
    beta = ex / ex.sum(1, keepdim=True)
    Z = (beta[:, :, None] * M).sum(1)
    bt = beta if beta_in is None else torch.from_numpy(beta_in)
    dbeta = torch.einsum("nd,npd->np", dZ, M)
    ds = bt * (dbeta - (bt * dbeta).sum(1, keepdim=True))
    dpre = ds[:, :, None] * u * (1.0 - v * v)
    dM = bt[:, :, None] * dZ[:, None, :] + dpre @ w.T
    dW = M.reshape(N * P, D).T @ dpre.reshape(N * P, -1)
    out = dict(Z=Z, beta=beta, dM=dM, dW=dW, db=dpre.sum((0, 1)), du=(ds[:, :, None] * v).sum((0, 1)))
    assert all(t.dtype == torch.float32 for t in out.values())
    return {k: t.numpy() for k, t in out.items()}


@pytest.mark.parametrize("P,D,A", SHAPES)
def test_fp32_restatement_within_bounds_dense(P, D, A):
    case = R.dense_case(65, P, D, A)
    got = restate(case)
    ratios = R.dense_ratios(case, got["Z"], got["beta"], got["dM"], (got["dW"], got["db"], got["du"]))
    print(P, D, A, {k: f"{x:.3g}" for k, x in ratios.items()})
    assert max(ratios.values()) <= 1.0, ratios
    # the block-by-block sums of dense_ratios are those of the one-shot reference
    ref = R.sem_ref(case, beta_in=got["beta"])
    for k, a, e in (("dW", ref.dW, ref.e_dW), ("db", ref.db, ref.e_db), ("du", ref.du, ref.e_du)):
        assert abs(R.ratio(got[k], a, e) - ratios[k]) <= 1e-6 * ratios[k] + 1e-12, k


@pytest.mark.parametrize("P,D,A", R.FAMILY_SHAPES)
def test_fp32_restatement_within_bounds_planted_and_wide_range(P, D, A):
    case = R.planted_case(1000, P, D, A)
    live = case["live"]
    got = restate(case)
    assert not got["dM"][np.setdiff1d(np.arange(1000), live)].any()
    ref = R.sem_ref(case, beta_in=got["beta"], nodes=live)
    assert ref.T == live.size
    ratios = R.planted_ratios(case, ref, *(got[k] for k in ("Z", "beta", "dM", "dW", "db", "du")), live)
    assert max(ratios.values()) <= 1.0, ratios
    case = R.wide_range_case(257, P, D, A)
    got = restate(case)
    ratios = R.dense_ratios(case, got["Z"], got["beta"], got["dM"])
    ref = R.sem_ref(case, beta_in=got["beta"])
    ratios.update(dW=R.ratio(got["dW"], ref.dW, ref.e_dW), db=R.ratio(got["db"], ref.db, ref.e_db),
                  du=R.ratio(got["du"], ref.du, ref.e_du))
    assert max(ratios.values()) <= 1.0, ratios


def test_fast_tanh_bound_covers_the_fp32_formula():
    """c_t u against the fp32 evaluation of 1 - 2 / (1 + exp(2x)) over +-20, and 1 <= c_t < 7.5."""
    x = np.linspace(-20, 20, 400001).astype(np.float32)
    t = torch.from_numpy(x)
    got = (1.0 - 2.0 / (1.0 + torch.exp(2.0 * t))).numpy().astype(np.float64)
    xd = x.astype(np.float64)
    v = np.tanh(xd)
    c_t = (1 - v * v) * (1 + 2 * np.abs(xd)) + 3 * (1 - v) + np.abs(v)
    assert c_t.max() < 7.5 and c_t.min() >= 1.0
    assert (np.abs(got - v) <= c_t * R.U).all()


# ------------------------------------------------------------------------------------------------ not too loose
@pytest.mark.parametrize("cell", R.CELLS, ids=lambda c: c.id)
def test_planted_bounds_see_a_dropped_node(cell):
    """Leaving any single live node out of the float64 sums moves at least one element of each of dW, db, du by more
    than its bound.  (At P = 1 beta = 1, ds = 0 and the three gradients vanish identically: nothing to drop.)"""
    case = R.planted_case(cell.N, cell.P, cell.D, cell.A, cell.flags)
    live = case["live"]
    assert {0, cell.N - 1} <= set(live.tolist()) and live.size <= 64
    ref = R.sem_ref(case, nodes=live)
    assert ref.T == live.size
    if cell.P == 1:
        assert not ref.dW.any() and not ref.ds.any()
        return
    M = R.up(case["M"][live])
    for i in range(live.size):
        assert (np.abs(M[i].T @ ref.dpre[i]) > ref.e_dW).any(), ("dW", live[i])
        assert (np.abs(ref.dpre[i].sum(0)) > ref.e_db).any(), ("db", live[i])
        assert (np.abs(ref.dsv[i].sum(0)) > ref.e_du).any(), ("du", live[i])


@pytest.mark.parametrize("P,D,A", SHAPES)
def test_dense_bounds_see_swapped_beta_and_shifted_rows(P, D, A):
    case, ref = R.small_ref("dense", 65, P, D, A)
    # Z of node n written to node n + 1
    assert ((np.abs(ref.Z[:-1] - ref.Z[1:]) > ref.e_Z[1:]).any(1)).all()
    # dM of a row written to the next row
    dM, e = ref.dM.reshape(-1, D), ref.e_dM.reshape(-1, D)
    assert ((np.abs(dM[:-1] - dM[1:]) > e[1:]).any(1)).all()
    if P == 1:
        return
    # the beta of the heaviest and the lightest meta-path of an unsaturated node swapped
    rows = np.arange(65)
    hi, lo = ref.beta.argmax(1), ref.beta.argmin(1)
    unsat = ref.beta[rows, hi] < 0.99
    assert unsat.sum() >= 60
    assert (ref.beta[rows, hi] - ref.beta[rows, lo] > ref.e_beta[rows, hi] + ref.e_beta[rows, lo])[unsat].all()


@pytest.mark.parametrize("P,D,A", [x for x in SHAPES if x[0] > 1])      # beta = 1 at P = 1
def test_dense_case_is_not_saturated(P, D, A):
    case = R.dense_case(1024, P, D, A)
    W, b, uo = R._f64(case)
    beta = R._fwd(R.up(case["M"]), W, b, uo).beta
    assert (beta.max(1) > 0.99).mean() < 0.05


def test_wide_range_case_underflows_and_cancels():
    case, ref = R.small_ref("wide_range", 257, 4, 64, 128)
    assert 79.9 < np.abs(ref.s).max() < 80.1
    assert (ref.beta < R.TINY).any() and (ref.g < R.U).any()


# ------------------------------------------------------------------------------------------------ the dispatch mirror
def test_mirrored_constants_match_the_source():
    src = open(_HIP).read()
    assert re.search(r"constexpr int ROWS = %d;" % R.ROWS, src)
    assert re.search(r"constexpr int kSemBwdBlocks = %d;" % R.BWD_BLOCKS, src)
    assert re.search(r"constexpr int kWideDChunk = %d;" % R.WIDE_D_CHUNK, src)
    assert re.search(r"static constexpr int AS = %d," % R.WIDE_A_SLICE, src)
    assert "N * P >= 64 * 1024" in src and R.B6_ROWS == 64 * 1024
    wave = r"han_grid_for\(a\.N \* a\.P, 64, 256 \* (\d)\);\s*HAN_DISPATCH_P\(a\.P, e = a\.launch\(sem_attn_fwd_%s<"
    chunk = r"sem_attn_fwd_%s<[A-Z, ]+>, han_grid_for\(a\.N, ROWS / a\.P, 256 \* (\d)\)"
    for name, pat in (("b6", wave % "wave_b6_kernel"), ("wave", wave % "wave_kernel"), ("block", chunk % "kernel"),
                      ("gen4", chunk % "gen_kernel"), ("gen8", chunk % "gen_kernel"), ("wide", chunk % "wide_kernel")):
        m = re.search(pat, src)
        assert m, name
        assert 256 * int(m.group(1)) == R.FWD_CAP[name], name
    assert len(re.findall(r"han_grid_for\([^;]*kSemBwdBlocks\)", src)) == 4      # every backward launcher


@pytest.mark.parametrize("cell", R.CELLS, ids=lambda c: c.id)
def test_cells_pass_their_loops_twice(cell):
    P, D, A, N = cell.P, cell.D, cell.A, cell.N
    fam = R.family(P, D, A)
    assert fam == {"exact": "wave", "b6": "wave"}.get(cell.kind, cell.kind)
    units, gf, gb = R.grids(N, P, D, A, cell.flags)
    b6 = R.uses_b6(N, P, D, A, cell.flags)
    assert b6 == (cell.kind == "b6")
    assert gb == R.BWD_BLOCKS and 2 * gb < units
    if cell.kind == "wave":
        assert N * P < R.B6_ROWS and gf == units
    else:
        assert gf == R.FWD_CAP["b6" if b6 else fam] and 2 * gf < units < 3 * gf
    if cell.kind == "exact":
        assert N * P > 2 * R.B6_ROWS
    if cell.kind == "b6":                        # two tiles per wave and pass: some waves end on a single one
        assert -(-units // gb) % 2 == 1 and units // gb % 2 == 0
    assert N * P < 140000
    npu = R.nodes_per_unit(P)
    tail = (N * P) % R.TILE if fam == "wave" else ((N % npu or npu) * P) % R.TILE
    assert tail != 0 or P in (16, 64)            # a partial 16-row tile ends the last unit
    if P == 1:
        assert (N * P) % R.TILE == 1
    # every planted position exists, and both grids have a live node in their second pass
    pos = R.planted_positions(N, P, D, A, cell.flags)
    npu = R.nodes_per_unit(P)
    assert any(gb <= n // npu < 2 * gb for n in pos)
    assert cell.kind == "wave" or any(gf <= n // npu < 2 * gf for n in pos)


def test_cells_cover_the_dispatch():
    names = set()
    for c in R.CELLS:
        names |= {n.split("<")[0] for n in R.kernel_names(c.N, c.P, c.D, c.A, c.flags)}
    assert names == {"fwd", "fwd_wave", "fwd_wave_b6", "bwd", "bwd_wave", "bwd_wave_b6", "bwd_pair_b6", "fwd_gen",
                     "bwd_gen", "fwd_wide", "bwd_wide"}
    src = open(_HIP).read()
    assert len(re.findall(r"__global__", src)) == len(names)
    g3b = {n for c in R.CELLS for n in R.kernel_names(c.N, c.P, c.D, c.A, c.flags) if "G3B" in n}
    assert {n[-6:] for n in g3b} == {"G3B=0>", "G3B=1>"}
    assert {R.wide_fwd_slice(c.A) for c in R.CELLS if c.kind == "wide"} == {64, 128, 192, 256}
    wide = [c for c in R.CELLS if c.kind == "wide"]
    assert any(c.A > R.WIDE_A_SLICE and c.D > R.WIDE_D_CHUNK and c.D % R.WIDE_D_CHUNK for c in wide)     # a short chunk
    assert any(c.D == 2 * R.WIDE_D_CHUNK for c in wide) and {c.D for c in wide} == {192, 256, 320}
    for P, N, A in R.SWITCH:
        assert R.uses_b6(N, P, 64, A, 0) == (N * P >= 65536)
