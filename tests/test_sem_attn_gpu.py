"""GPU tests of han_amd/csrc/sem_attn.hip (K3, semantic attention) through han_amd.ops.sem_attn_fwd / sem_attn_bwd: every
one of its eleven kernels, per row, past every row loop.

Every comparison is elementwise |gpu - float64| <= e with the bound e of tests/sem_attn_ref.py (counts of fp32 roundings,
derived there; tests/test_sem_attn_ref_host.py checks reference, bounds and cases without a GPU).  The backward reference
starts from the beta the GPU forward returned.  One entry per cell of the dispatch (sem_attn_ref.CELLS), each at the
smallest N at which every block of the forward and of the backward grid passes its row loop 2-3 times:
  dense    every node live: Z, beta, the row sums of beta and dM of every row (the run-time-width cells take the backward
           on the first 2 * 256 + 5 chunks, which is past its loop, to keep the float64 work in seconds);
  planted  dZ nonzero on at most 64 nodes placed at the ends of the grid passes, tiles, lane groups and chunks: Z, beta,
           dM of the live nodes, dW, db, du against bounds that count T P roundings; dM of every dead node exactly 0.
Further: both sides of the switch to the bf16 x 6 kernels, scores up to +-80, N in {1, 15, 16, 17, 63, 65} (and around one
chunk for P not a power of two), NaN-poisoned outputs and workspace, determinism, FLAG_K3_EXACT_PIPE below the switch.

Largest err / bound measured on an MI355X (gfx950), per kernel instance over all of its cases (the template arguments
name the instance: sem_attn_fwd_kernel<CA> is "fwd<CA>", sem_attn_bwd_wave_b6_kernel<CA, P, G3B> "bwd_wave_b6<...>", and so
on; profiles/r16_k3_parity_ratios.json holds the same table with (P, D, A, N, flags) of every case).  The rows are also
the list of kernel instances that ran -- all eleven __global__ kernels of sem_attn.hip, both G3B values and the pair kernel
-- and the N are those of their cases: the five-digit ones are past the row loops (2 * cap + 5 units of 64 / P nodes).

    forward kernel                 Z        beta     sum_beta  N of the cases that ran (e: with FLAG_K3_EXACT_PIPE)
    fwd<CA=1>                      8e-04    0.93     7e-04     1 2 3 15 16 17 63 65 257 1542 18496
    fwd<CA=2>                      9e-04    0.55     3e-04     1 15 16 17 21 22 43 63 65 257 1542 13872 32367
    fwd_gen<CA=1,DT=8>             7e-04    8e-04    6e-05     32937
    fwd_gen<CA=2,DT=8>             4e-04    5e-04    5e-05     21615
    fwd_gen<CA=3,DT=4>             5e-04    7e-04    1e-04     16469
    fwd_gen<CA=3,DT=8>             2e-04    0.43     7e-05     1 12 13 15 16 17 25 63 65 257 8235
    fwd_gen<CA=4,DT=4>             4e-04    8e-04    1e-04     1 15 16 17 21 22 43 63 65 257 4118 21615
    fwd_gen<CA=4,DT=8>             2e-04    4e-04    6e-05     12352
    fwd_wave<CA=1,P=16>            0.0011   0.87     3e-04     1 15 16 17 63 65 257 2070 4095 8214e
    fwd_wave<CA=1,P=1>             0        0        0         1 15 16 17 63 65 257 33105 131409e
    fwd_wave<CA=1,P=2>             0.0014   0.0018   2e-04     16553 65705e
    fwd_wave<CA=1,P=4>             0.0011   0.0018   2e-04     8277 32853e
    fwd_wave<CA=1,P=8>             9e-04    0.0017   2e-04     4139 16427e
    fwd_wave<CA=2,P=16>            5e-04    0.001    1e-04     2070 8214e
    fwd_wave<CA=2,P=1>             0        0        0         33105 65535 131409e
    fwd_wave<CA=2,P=2>             0.0011   0.0011   9e-05     16553 65705e
    fwd_wave<CA=2,P=4>             8e-04    0.77     1e-04     1 15 16 17 63 65 257 8277 32853e
    fwd_wave<CA=2,P=8>             6e-04    0.0011   2e-04     4139 16427e
    fwd_wave_b6<CA=1,P=16>         8e-04    0.0021   3e-04     4096 6166
    fwd_wave_b6<CA=1,P=1>          0        0        0         98641
    fwd_wave_b6<CA=1,P=2>          0.0016   0.56     1e-04     32800 49321
    fwd_wave_b6<CA=1,P=4>          1e-03    0.0017   2e-04     24661
    fwd_wave_b6<CA=1,P=8>          7e-04    0.0015   2e-04     12331
    fwd_wave_b6<CA=2,P=16>         4e-04    0.001    1e-04     6166
    fwd_wave_b6<CA=2,P=1>          0        0        0         65536 98641
    fwd_wave_b6<CA=2,P=2>          8e-04    1e-03    9e-05     49321
    fwd_wave_b6<CA=2,P=4>          6e-04    0.001    1e-04     24661
    fwd_wave_b6<CA=2,P=8>          7e-04    0.97     2e-04     8200 12331
    fwd_wide<CA=1>                 4e-04    5e-04    6e-05     2054 32853
    fwd_wide<CA=2>                 2e-04    0.58     2e-05     1 15 16 17 63 65 257 43119
    fwd_wide<CA=3>                 1e-04    0.23     4e-05     1 15 16 17 21 22 43 63 65 257 4107
    fwd_wide<CA=4>                 4e-05    1e-04    2e-05     2054
    backward kernel                dM       dW       db       du
    bwd<CA=1>                      0.0114   0.0044   0.0021   0.002    1 2 3 15 16 17 63 65 257 1542 18496
    bwd<CA=2>                      0.0122   0.0121   0.0029   0.0023   1 15 16 17 21 22 43 63 65 257 1542 13872 32367
    bwd_gen<DT=4>                  0.0036   0.0394   0.0121   0.0048   1 15 16 17 21 22 43 63 65 257 4118 16469 21615
    bwd_gen<DT=8>                  0.0043   0.0116   0.0033   0.0041   1 12 13 15 16 17 25 63 65 257 8235 12352 21615 32937
    bwd_pair_b6<P=2>               0.011    0.0031   0.0019   0.0016   49321
    bwd_pair_b6<P=8>               0.0121   0.0015   7e-04    8e-04    8200 12331
    bwd_wave<CA=1,P=16>            0.0179   0.0334   0.0111   0.0034   1 15 16 17 63 65 257 2070 4095 8214e
    bwd_wave<CA=1,P=1>             0        0        0        0        1 15 16 17 63 65 257 33105 131409e
    bwd_wave<CA=1,P=2>             0.0162   0.0036   0.0022   0.0018   16553 65705e
    bwd_wave<CA=1,P=4>             0.014    0.0026   0.0013   0.001    8277 32853e
    bwd_wave<CA=1,P=8>             0.014    0.0024   6e-04    8e-04    4139 16427e
    bwd_wave<CA=2,P=16>            0.0149   0.0015   5e-04    6e-04    2070 8214e
    bwd_wave<CA=2,P=1>             0        0        0        0        33105 65535 131409e
    bwd_wave<CA=2,P=2>             0.0153   0.0044   0.0018   0.0019   16553 65705e
    bwd_wave<CA=2,P=4>             0.0174   0.0537   0.0099   0.0059   1 15 16 17 63 65 257 8277 32853e
    bwd_wave<CA=2,P=8>             0.0134   0.0021   8e-04    9e-04    4139 16427e
    bwd_wave_b6<CA=1,P=1,G3B=1>    0        0        0        0        98641
    bwd_wave_b6<CA=1,P=16,G3B=0>   0.0128   0.0011   4e-04    5e-04    6166
    bwd_wave_b6<CA=1,P=16,G3B=1>   0.0128   0.0011   4e-04    5e-04    4096 6166
    bwd_wave_b6<CA=1,P=2,G3B=1>    0.0137   0.0031   9e-04    0.0017   32800 49321
    bwd_wave_b6<CA=1,P=4,G3B=1>    0.0122   0.0019   9e-04    9e-04    24661
    bwd_wave_b6<CA=1,P=8,G3B=1>    0.0112   0.0017   5e-04    1e-03    12331
    bwd_wave_b6<CA=2,P=1,G3B=1>    0        0        0        0        65536 98641
    bwd_wave_b6<CA=2,P=16,G3B=1>   0.0101   9e-04    3e-04    4e-04    6166
    bwd_wave_b6<CA=2,P=2,G3B=1>    0.011    0.0031   0.0019   0.0016   49321
    bwd_wave_b6<CA=2,P=4,G3B=0>    0.0114   0.0023   9e-04    0.0011   24661
    bwd_wave_b6<CA=2,P=4,G3B=1>    0.0114   0.0023   9e-04    0.0011   24661
    bwd_wave_b6<CA=2,P=8,G3B=0>    0.0064   2e-05    8e-06    3e-06    8200
    bwd_wave_b6<CA=2,P=8,G3B=1>    0.0121   0.0015   7e-04    8e-04    8200 12331
    bwd_wide                       0.0022   0.0264   0.004    0.0034   1 15 16 17 21 22 43 63 65 257 2054 4107 32853 43119

Every ratio is <= 1: no kernel bug was found, and sem_attn.hip is unchanged.  A beta ratio between 0.2 and 1 comes from the
wide-range cases, where a beta below 2^-126 is flushed to zero and the bound is TINY alone; at P = 1 beta = 1, Z = M and
dM = dZ hold exactly and dW, db, du are exact zeros.  The worst-case bounds lie two to three orders of magnitude above
the errors of a correct kernel, as such bounds do; what they still exclude is asserted in the host file (a dropped node, a
swapped beta, a shifted row).  The 205 cases of this file take 37 s with 16 host threads, the slowest 1.4 s, nearly all of
it the float64 reference; a forward + backward pair of the largest case takes a few milliseconds on the GPU.
"""
import json
import os

import numpy as np
import pytest
import torch

from tests import sem_attn_ref as R

pytestmark = pytest.mark.gpu

_SEEN = {}
_CELLS = {}


def _note(tag, ratios):
    for k, v in ratios.items():
        _SEEN[(tag, k)] = max(_SEEN.get((tag, k), 0.0), v)
    print(tag, {k: f"{v:.3g}" for k, v in ratios.items()})


@pytest.fixture(scope="module", autouse=True)
def _report():
    """Prints the largest err / bound per kernel and quantity when the module is done (pytest -s); HAN_RATIO_JSON names
    a file that receives the same table."""
    yield
    for (tag, k), v in sorted(_SEEN.items()):
        print(f"{tag:40s} {k:8s} {v:.3g}")
    for tag, cells in sorted(_CELLS.items()):
        print(f"{tag:40s} {' '.join(sorted(cells))}")
    path = os.environ.get("HAN_RATIO_JSON")
    if path:
        table = {f"{tag} | {k}": v for (tag, k), v in sorted(_SEEN.items())}
        table.update({f"{tag} | cells (P,D,A,N,flags)": sorted(cells) for tag, cells in sorted(_CELLS.items())})
        with open(path, "w") as f:
            json.dump(table, f, indent=1)


def _note_both(N, P, D, A, flags, ratios):
    fwd, bwd = R.kernel_names(N, P, D, A, flags)
    for tag in (fwd, bwd):
        _CELLS.setdefault(tag, set()).add(f"({P},{D},{A},{N},{flags})")
    _note(fwd, {k: v for k, v in ratios.items() if k in ("Z", "beta", "sum_beta")})
    _note(bwd, {k: v for k, v in ratios.items() if k in ("dM", "dW", "db", "du")})


def _gpu(case, dev):
    return {k: torch.from_numpy(np.ascontiguousarray(case[k])).to(dev) for k in ("M", "w", "b", "u", "dZ")}


def _fwd(t, flags=0):
    from han_amd import ops
    return ops.sem_attn_fwd(t["M"], t["w"], t["b"], t["u"], flags=flags)


def _bwd(t, beta, flags=0, out=None, n=None):
    from han_amd import ops
    M, dZ = (t["M"], t["dZ"]) if n is None else (t["M"][:n], t["dZ"][:n])
    return ops.sem_attn_bwd(M, t["w"], t["b"], t["u"], beta if n is None else beta[:n], dZ, out=out, flags=flags)


def _np(*ts):
    return tuple(x.cpu().numpy() for x in ts)


def _dense(dev, case, flags, n_bwd=None, grads=False):
    """Forward and backward of a dense case -> the ratios of dense_ratios."""
    t = _gpu(case, dev)
    Z, beta = _fwd(t, flags)
    dM, dW, db, du = _bwd(t, beta, flags, n=n_bwd)
    Z, beta, dM, dW, db, du = _np(Z, beta, dM, dW, db, du)
    assert all(np.isfinite(x).all() for x in (Z, beta, dM, dW, db, du))
    return R.dense_ratios(case, Z, beta, dM, (dW, db, du) if grads else None)


def _planted(dev, case, flags, out=None):
    """Forward and backward of a planted case -> (ratios, the six outputs as tensors)."""
    t = _gpu(case, dev)
    Z, beta = _fwd(t, flags)
    outs = (Z, beta) + tuple(_bwd(t, beta, flags, out=out))
    Zn, bn, dM, dW, db, du = _np(*outs)
    live = case["live"]
    dead = np.ones(Zn.shape[0], dtype=bool)
    dead[live] = False
    assert not dM[dead].any(), "dM of a node with dZ = 0 must be exactly 0"
    ref = R.sem_ref(case, beta_in=bn, nodes=live)
    assert ref.T == live.size
    return R.planted_ratios(case, ref, Zn, bn, dM, dW, db, du, live), outs


def test_flag_values_mirror_ops():
    from han_amd import ops
    assert (ops.FLAG_K3_EXACT_PIPE, ops.FLAG_K3_PAIRS, ops.FLAG_K3_G3_F32) == (R.FLAG_EXACT, R.FLAG_PAIRS, R.FLAG_G3_F32)


# ------------------------------------------------------------------------------------------------ the cells
@pytest.mark.parametrize("cell", R.CELLS, ids=lambda c: c.id)
def test_dense_every_row(dev, cell):
    P, D, A, N = cell.P, cell.D, cell.A, cell.N
    case = R.cached_case("dense", N, P, D, A)
    n_bwd = R.loop_n(P, R.BWD_BLOCKS) if cell.kind == "wide" else None
    ratios = _dense(dev, case, cell.flags, n_bwd)
    _note_both(N, P, D, A, cell.flags, ratios)
    assert max(ratios.values()) <= 1.0, ratios


@pytest.mark.parametrize("cell", R.CELLS, ids=lambda c: c.id)
def test_planted_nodes_past_the_loops(dev, cell):
    P, D, A, N = cell.P, cell.D, cell.A, cell.N
    case = R.cached_case("planted", N, P, D, A, cell.flags)
    ratios, _ = _planted(dev, case, cell.flags)
    _note_both(N, P, D, A, cell.flags, ratios)
    assert max(ratios.values()) <= 1.0, ratios


@pytest.mark.parametrize("P,N,A", R.SWITCH)
def test_both_sides_of_the_pipe_switch(dev, P, N, A):
    """R = 65535 / 65536 rows: the last fp32-pipe size and the first bf16 x 6 one."""
    ratios = _dense(dev, R.cached_case("dense", N, P, 64, A), 0)
    _note_both(N, P, 64, A, 0, ratios)
    assert max(ratios.values()) <= 1.0, ratios
    ratios, _ = _planted(dev, R.cached_case("planted", N, P, 64, A, 0), 0)
    _note_both(N, P, 64, A, 0, ratios)
    assert max(ratios.values()) <= 1.0, ratios


# ------------------------------------------------------------------------------------------------ per family
@pytest.mark.parametrize("P,D,A,N,flags", R.WIDE_RANGE)
def test_wide_score_range(dev, P, D, A, N, flags):
    """Scores up to +-80: beta underflows, 1 - v^2 cancels; no NaN / Inf (asserted in _dense), every ratio <= 1."""
    ratios = _dense(dev, R.cached_case("wide_range", N, P, D, A), flags, grads=True)
    _note_both(N, P, D, A, flags, ratios)
    assert max(ratios.values()) <= 1.0, ratios


SMALL = [(P, D, A, N) for (P, D, A) in R.FAMILY_SHAPES for N in R.small_ns(P)]


@pytest.mark.parametrize("P,D,A,N", SMALL)
def test_small_n(dev, P, D, A, N):
    """A single node, partial tiles, partial chunks and their padding rows; dW, db, du with every node live."""
    ratios = _dense(dev, R.cached_case("dense", N, P, D, A), 0, grads=True)
    _note_both(N, P, D, A, 0, ratios)
    assert max(ratios.values()) <= 1.0, ratios


def _family_cells():
    """The first cell of every kernel instance family (and of every flag)."""
    seen, out = set(), []
    for c in R.CELLS:
        key = (c.kind, c.flags, c.P in R.POW2, c.P > 16)
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


FAMILY_CELLS = _family_cells()


def _poison(dev, case):
    """0xFF bytes (NaN as fp32) in the cached K3 workspace and in the blocks the next outputs are carved from; returns
    NaN-filled dw, db, du for `out=`."""
    from han_amd import ops
    for (_, tag), ws in ops._workspaces.items():
        if tag.startswith("sem"):
            ws.fill_(0xFF)
    N, P, D = case["M"].shape
    junk = [torch.full(s, float("nan"), device=dev) for s in ((N, P, D), (N, D), (N, P))]
    del junk
    return tuple(torch.full(case[k].shape, float("nan"), device=dev) for k in ("w", "b", "u"))


@pytest.mark.parametrize("cell", FAMILY_CELLS, ids=lambda c: c.id)
def test_poisoned_outputs_and_deterministic(dev, cell):
    """Two plain calls give identical bits for all outputs; a third one with NaN in the slab workspace, in the memory the
    outputs are carved from and in the `out=` tensors gives them again: every slab row and output element is written."""
    P, D, A, N = cell.P, cell.D, cell.A, cell.N
    case = R.cached_case("planted", N, P, D, A, cell.flags)
    _, a = _planted(dev, case, cell.flags)
    _, b = _planted(dev, case, cell.flags)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    go = _poison(dev, case)
    ratios, c = _planted(dev, case, cell.flags, out=go)
    assert c[3] is go[0] and c[4] is go[1] and c[5] is go[2]
    assert all(torch.isfinite(x).all() for x in c)
    assert all(torch.equal(x, y) for x, y in zip(a, c))
    assert max(ratios.values()) <= 1.0, ratios


@pytest.mark.parametrize("P,A", [(1, 64), (4, 128), (16, 64)])
def test_exact_pipe_flag_below_the_switch_is_the_default(dev, P, A):
    """Below 65 536 rows FLAG_K3_EXACT_PIPE selects the kernels flags 0 selects: the same bits."""
    N = R.loop_n(P, R.BWD_BLOCKS)
    assert N * P < R.B6_ROWS
    case = R.cached_case("planted", N, P, 64, A, 0)
    _, a = _planted(dev, case, 0)
    _, b = _planted(dev, case, R.FLAG_EXACT)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
