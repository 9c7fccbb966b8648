"""tests/k1_cases.py without a GPU: its checks against the CPU stand-ins (references, mask indexing, seed_dev, bf16
rounding and keep-bit handling are self-consistent), the exact-grid precondition of every case, and -- from the
library's host-side size queries -- that every forward case of tests/test_project_gpu.py reaches the path it
declares."""
import numpy as np
import pytest
import torch

from tests import cpu_backend, k1_cases as kc, rng_ref

SMALL = [c for c in kc.ALL if c.n <= kc.CPU_MAX_ROWS]
CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def lib():
    from han_amd import _lib
    _lib.build()
    return _lib.load()


@pytest.mark.parametrize("c", SMALL, ids=kc.ids(SMALL))
def test_checks_hold_against_the_cpu_stand_ins(c):
    kc.check(cpu_backend, CPU, c)


def test_the_small_cases_cover_every_check_and_mode():
    kinds = {(c.kind, c.random) for c in SMALL}
    assert {(k, r) for k in ("fwd", "dw", "dx") for r in (False, True)} <= kinds
    assert any(c.seed_dev for c in SMALL) and any(c.fts and c.bf16_table for c in SMALL)
    assert any(c.row_offset > 2 ** 31 for c in SMALL)


def test_a_wrong_value_fails_the_checks():
    """the checks do fail: one element off by one grid unit, one keep bit flipped, one dropped term"""
    class Off:
        def __init__(self, fn):
            self.fn = fn

        def project_fwd(self, *a, **k):
            out = list(cpu_backend.project_fwd(*a, **k))
            out[0] = self.fn(out[0])
            return tuple(out)

        def project_bwd_input(self, *a, **k):
            return self.fn(cpu_backend.project_bwd_input(*a, **k))

    def unit(t):
        t = t.clone()
        t[-1, -1] += kc.GX * kc.GW
        return t

    def keepbit(t):
        t = t.clone()
        v = t.view(torch.int32)
        v[-1, -1] ^= 1
        return t

    def tiny(t):       # far below any relative-to-max tolerance
        return t * (1 + 2.0 ** -12)

    exact = next(c for c in kc.FWD_PLAIN if (c.n, c.f) == (130, 77) and not c.random and not c.drop)
    stamped = next(c for c in kc.FWD_PLAIN if c.fts and not c.random and not c.bf16_table)
    rand = next(c for c in kc.FWD_PLAIN if c.random and not c.drop)
    rdx = next(c for c in kc.DX if c.random and not c.drop)
    for case, fn in ((exact, unit), (stamped, keepbit), (stamped, unit), (rand, tiny), (rdx, tiny)):
        with pytest.raises(AssertionError):
            kc.check(Off(fn), CPU, case)


def test_block_masks_are_the_reference_masks():
    for K in (1, 2, 4, 8, 16):
        want = rng_ref.seq_mask(0xABCDEF0123, 40, 19, K, 0.5, row_offset=kc.BIG_OFFSET)
        got = kc.seq_masks(0xABCDEF0123, 0, 40, 19, K, 0.5, kc.BIG_OFFSET)
        assert np.array_equal(got, want.astype(bool))
        part = kc.seq_masks(0xABCDEF0123, 7, 23, 19, K, 0.5, kc.BIG_OFFSET)
        assert np.array_equal(part, got[:, 7:23])


@pytest.mark.parametrize("c", kc.ALL, ids=kc.ids(kc.ALL))
def test_exact_grid_precondition(c):
    """make_inputs asserts, in float64 and from the inputs alone, that every term sum stays below 2^24 grid units"""
    arrs = kc.make_inputs(c)
    assert all(np.isfinite(a).all() for a in arrs)
    if c.path == "pipe" and not c.random and not c.xbf:      # the mid term of the three-way split is not zero
        m = np.abs(arrs[0] / kc.GX)
        assert (m >= 257).all() and (m % 2 == 1).all()


@pytest.mark.parametrize("c", kc.FWD_ALL, ids=kc.ids(kc.FWD_ALL))
def test_forward_cases_reach_the_path_they_declare(lib, c):
    assert kc.forward_path(c.n, c.f, c.P) == c.path
    if c.kind == "multi":
        assert kc.forward_path(c.n, c.f, 1) == "pipe"
    if c.keep_table:
        assert lib.han_project_keep_bytes(c.n, c.f, c.f, 8, 8) == c.n * c.f + 128


def test_forward_path_boundaries(lib):
    assert kc.forward_path(32640, 128) == "split" and kc.forward_path(32641, 128) == "pipe"
    assert kc.forward_path(16383, 64) == "plain" and kc.forward_path(16384, 64) == "pipe"
    assert kc.forward_path(16383, 64, 4) == "plain" and kc.forward_path(16384, 64, 4) == "pipe"
    assert kc.forward_path(3000, 256, 2) == "split"
    assert lib.han_project_keep_bytes(32767, 8, 8, 8, 8) == 0 and lib.han_project_keep_bytes(32768, 8, 8, 8, 8) > 0


def test_size_queries_of_an_empty_input(lib):
    """no rows: no workspace and no table at any width (the split-F geometry divides by the row-tile count, so F >= 128
    must not reach it); ops.project_fwd asks these before it sees that N == 0"""
    for f in (5, 127, 128, 1870):
        assert lib.han_project_fwd_workspace(0, f, 8, 8) == 0 and lib.han_project_fwd_multi_workspace(0, f, 8, 8, 3) == 0
        assert lib.han_project_keep_bytes(0, f, f, 8, 8) == 0 and lib.han_project_bwd_workspace(0, f, 8, 8) == f * 64 * 4


@pytest.mark.parametrize("n,f", [(20000, 1868), (17000, 256), (16500, 200), (16514, 256), (16514, 328),
                                 (16584, 256), (20000, 132)])
def test_shapes_the_matrix_pipe_tests_used_to_run_are_split(lib, n, f):
    """test_gpu_parity.py ran its matrix-pipe and fused-launch tests at these shapes: with F >= 128 the forward is
    whole-F only from N = 32641, below that HAN_FLAG_K1_MATRIX_PIPE is ignored and project_fwd_multi loops over the
    per-meta-path split kernel.  (Why those parametrisations moved.)"""
    assert kc.forward_path(n, f) == "split" and kc.forward_path(n, f, 4) == "split"
