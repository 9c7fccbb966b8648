"""K1 (han_amd/csrc/project.hip) kernel by kernel: every entry point at the shapes that select each kernel
instantiation, against float64 references -- EQUAL on exact-grid inputs, within the summation-order-free fp32 bound
on random ones (tests/k1_cases.py has the cases, the inputs, the references and the checks).

Every forward case asserts the path the library's own size queries name for its shape before it launches."""
import pytest
import torch

from tests import k1_cases as kc

pytestmark = pytest.mark.gpu


def _run(dev, c):
    from han_amd import ops
    if c.kind in ("fwd", "multi"):
        assert kc.forward_path(c.n, c.f, c.P) == c.path, c.id
        if c.kind == "multi":      # the single-path call the fused rows are compared with is on the matrix pipe too
            assert kc.forward_path(c.n, c.f, 1) == "pipe", c.id
    kc.check(ops, dev, c)
    torch.cuda.synchronize()


@pytest.mark.parametrize("c", kc.FWD_PLAIN, ids=kc.ids(kc.FWD_PLAIN))
def test_project_fwd_plain(dev, c):
    """project_fwd_kernel<F', DROP, MT = 2>, whole-F: scalar and vector loads, strided / misaligned / bf16 X, every
    head shape on both table types, row offsets beyond 2^31 and a device seed word."""
    _run(dev, c)


@pytest.mark.parametrize("c", kc.FWD_SPLIT, ids=kc.ids(kc.FWD_SPLIT))
def test_project_fwd_split(dev, c):
    """project_fwd_kernel<F', DROP, MT = 1> over F chunks + project_finish_kernel."""
    _run(dev, c)


@pytest.mark.parametrize("c", kc.FWD_PIPE, ids=kc.ids(kc.FWD_PIPE))
def test_project_fwd_pipe(dev, c):
    """project_fwd_b6_kernel (fp32 X under FLAG_K1_MATRIX_PIPE, bf16 X and dropout by default; with and without the
    keep table; 4 and 8 waves), project_scores_kernel behind it, and the exact-fp32 kernel on the same shapes."""
    _run(dev, c)


@pytest.mark.parametrize("c", kc.FWD_MULTI, ids=kc.ids(kc.FWD_MULTI))
def test_project_fwd_multi_fused(dev, c):
    """project_fwd_b6_multi_kernel: 4 and 2 meta-paths per block, groups in grid.y, an odd last meta-path, bf16 X and
    table; bit for bit the single-path matrix-pipe kernel."""
    _run(dev, c)


@pytest.mark.parametrize("c", kc.DW, ids=kc.ids(kc.DW))
def test_project_bwd_dw(dev, c):
    """project_bwd_kernel: row counts around the reduction step, widths around the 128-row tile, every head shape's
    accumulator selection under dropout, strided / misaligned / bf16 X, out= into a slice."""
    _run(dev, c)


@pytest.mark.parametrize("c", kc.DW_KEEP, ids=kc.ids(kc.DW_KEEP))
def test_project_bwd_dw_keep_table(dev, c):
    """project_bwd_blk_kernel through the forward's keep table, against float64 and the hash-regenerating kernel."""
    _run(dev, c)


@pytest.mark.parametrize("c", kc.DX, ids=kc.ids(kc.DX))
def test_project_bwd_input(dev, c):
    """project_bwd_input_kernel: partial row and feature tiles, every head shape with and without dropout, the
    strided out=dXin[:, p, :] of the model, row offset and device seed word."""
    _run(dev, c)
