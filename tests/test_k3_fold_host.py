"""Host side of the K3 backward that also runs the row-local K2 backward (HeteGAT_multi.fold_k3, han_sem_attn_bwd_rows):
CPU tensors never reach the fused op, the C entry refuses what it does not take before any launch, ABI 15."""
import ctypes

import numpy as np
import pytest
import torch

from tests.helpers import make_problem
from tests.test_host_cpu import _cpu_graphs, _cpu_model, cpu_ops  # noqa: F401  (fixture)


def test_abi_is_15():
    from han_amd import _lib
    assert _lib.ABI_VERSION == 15
    assert _lib.load().han_abi_version() == 15
    assert "han_sem_attn_bwd_rows" in _lib.SIGNATURES and "han_sem_attn_bwd_rows_workspace" in _lib.SIGNATURES


def test_cpu_epoch_is_the_same_with_fold_k3_set(cpu_ops, monkeypatch):
    """With the CPU stand-in backend a trainer epoch with fold_k3 set gives the bits of one with it unset, and the
    fused op is never called."""
    from han_amd import rng as hrng
    from han_amd.trainer import HANTrainer

    def never(*a, **k):
        raise AssertionError("ops.sem_attn_bwd_rows was reached with CPU tensors")

    monkeypatch.setattr(cpu_ops, "sem_attn_bwd_rows", never)
    prob = make_problem(31, 40, 12, 2, 3, [0.1, 0.4])
    x = torch.tensor(prob["x"][0], dtype=torch.float32)
    out = []
    for fold in (True, False):
        model, _ = _cpu_model(prob)
        hrng.manual_seed(123)
        tr = HANTrainer(model, [x, x], _cpu_graphs(prob), torch.tensor(prob["labels"], dtype=torch.int32),
                        torch.tensor(prob["mask"].astype(np.uint8)), torch.tensor((~prob["mask"]).astype(np.uint8)),
                        attn_drop=0.6, ffd_drop=0.6)
        assert model.fold_k3 is True          # the trainer sets it, as it does direct_grads
        model.fold_k3 = fold
        vals = [float(v) for v in tr.epoch()]
        out.append((vals, model.flat.clone(), model.flat_grad.clone()))
    assert out[0][0] == out[1][0]
    assert torch.equal(out[0][1], out[1][1]) and torch.equal(out[0][2], out[1][2])


def _call(lib, N, P, D, A, null=None, K=8, FP=8, dtype=0, act=1, flags=0):
    """han_sem_attn_bwd_rows with fake (never dereferenced) device pointers: every refusal is decided on the host."""
    fake = 0x1000
    n_p = max(P, 1)
    arr = lambda: (ctypes.c_void_p * n_p)(*([fake] * n_p))
    args = {k: fake for k in ("M", "w", "b", "u", "beta", "dZ", "c", "dw", "db", "du", "dc", "ws")}
    ptrs = {k: arr() for k in ("aggp", "tsum", "f1", "lse", "gs", "df1")}
    if null in args:
        args[null] = None
    elif null in ptrs:
        ptrs[null] = None
    elif null is not None:                      # "aggp[1]": one entry of a pointer array
        name, i = null[:-3], int(null[-2])
        ptrs[name][i] = None
    return lib.han_sem_attn_bwd_rows(args["M"], args["w"], args["b"], args["u"], args["beta"], args["dZ"], ptrs["aggp"],
                                     ptrs["tsum"], ptrs["f1"], ptrs["lse"], args["c"], ptrs["gs"], ptrs["df1"],
                                     args["dw"], args["db"], args["du"], args["dc"], args["ws"], 1 << 30, N, P, D, A, K, FP,
                                     dtype, act, flags, None)


@pytest.mark.parametrize("null", ["M", "w", "b", "u", "beta", "dZ", "c", "dw", "db", "du", "dc", "ws",
                                  "aggp", "tsum", "f1", "lse", "gs", "df1", "aggp[1]", "gs[3]", "df1[0]"])
def test_entry_refuses_null_pointers(null):
    from han_amd import _lib
    assert _call(_lib.load(), 1 << 20, 4, 64, 128, null=null) == -1          # HAN_E_BADARG


@pytest.mark.parametrize("why,kw", [
    ("P = 3", dict(N=1 << 20, P=3, D=64, A=128)),
    ("D = 128", dict(N=1 << 20, P=4, D=128, A=128)),
    ("N * P < 65 536", dict(N=16383, P=4, D=64, A=128)),
    ("A = 192", dict(N=1 << 20, P=4, D=64, A=192)),
    ("P = 8", dict(N=1 << 20, P=8, D=64, A=128)),
    ("4 x 16 heads", dict(N=1 << 20, P=4, D=64, A=128, K=4, FP=16)),
    ("bf16 tables", dict(N=1 << 20, P=4, D=64, A=128, dtype=1)),
    ("another activation code", dict(N=1 << 20, P=4, D=64, A=128, act=2)),
    ("exact-pipe flag", dict(N=1 << 20, P=4, D=64, A=128, flags=8)),
    ("pairs flag", dict(N=1 << 20, P=4, D=64, A=128, flags=16)),
    ("fp32 G3 flag", dict(N=1 << 20, P=4, D=64, A=128, flags=32)),
    ("table offsets beyond 32 bits", dict(N=12_000_000, P=4, D=64, A=128)),
])
def test_entry_refuses_other_shapes_without_a_launch(why, kw):
    """No GPU is needed to be refused: nothing is launched (the pointers are not device memory)."""
    from han_amd import _lib
    assert _call(_lib.load(), **kw) == _lib.E_UNSUPPORTED, why


def test_workspace_grows_by_the_dc_columns():
    from han_amd import _lib
    lib = _lib.load()
    for P in (1, 2, 4):
        for A in (64, 128):
            assert lib.han_sem_attn_bwd_rows_workspace(1 << 20, P, 64, A) == \
                lib.han_sem_attn_bwd_workspace(1 << 20, P, 64, A) + 256 * 64 * P * 4


def test_fused_kernels_use_no_scratch(tmp_path):
    """The fused kernel runs one wave per SIMD on (nearly) the whole register file, and what keeps it there is fragile
    (csrc/sem_attn_fold.h: fold_lane).  The code objects inside the built library must say that none of its six forms
    uses private memory or spills a vector register."""
    import os
    import struct
    import subprocess
    from han_amd import _lib
    from tools import kernel_diff
    fat = str(tmp_path / "fatbin")
    subprocess.run([kernel_diff._tool("llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, _lib.LIB_PATH,
                    str(tmp_path / "copy.so")], check=True)
    blob = open(fat, "rb").read()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    found = {}
    at = blob.find(magic)
    while at >= 0:                                   # one bundle per source: [magic][n][offset, size, len, triple] x n
        n, = struct.unpack_from("<Q", blob, at + len(magic))
        pos = at + len(magic) + 8
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", blob, pos)
            triple = blob[pos + 24:pos + 24 + tl].decode()
            pos += 24 + tl
            if "gfx950" in triple and size:
                co = str(tmp_path / f"co_{at}.o")
                open(co, "wb").write(blob[at + off:at + off + size])
                notes = subprocess.run([kernel_diff._tool("llvm-readelf"), "--notes", co], capture_output=True, text=True,
                                       check=True).stdout
                found.update({k: v for k, v in kernel_diff.parse_notes(notes).items() if "b6_fold_kernel" in k})
        at = blob.find(magic, at + 1)
    assert len(found) == 6, sorted(found)            # A in {64, 128} x P in {1, 2, 4}
    for name, res in found.items():
        assert res["private_segment_fixed_size"] == 0 and res["vgpr_spill_count"] == 0, (name, res)
