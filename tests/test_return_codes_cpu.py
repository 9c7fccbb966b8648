"""The validation order of the K1 and classifier entry points, pinned through their return codes.

Every call here returns while the library still validates its arguments, before any launch: the pointers are dummy
values, not memory.  The base arguments of each entry point already end in a validation error (a split-F shape
without its workspace, a classifier without workspace bytes); a case overrides what must be seen first, or names the
shape it needs.  The module skips itself where a launch could actually start."""
import pytest
import torch

BADARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
EXACT_PIPE, MATRIX_PIPE = 2, 4
PTR = 0x10000          # non-null, 16-byte aligned, never dereferenced
AMPLE = 1 << 40


def ONE_IMAGE(lib):     # the W image of ONE meta-path of the PIPE shape: too small for the fused launch of three
    return lib.han_project_fwd_workspace(PIPE["N"], PIPE["F"], 8, 8)


pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="dummy pointers: only where no launch can start")


@pytest.fixture(scope="module")
def lib():
    from han_amd import _lib
    _lib.build()
    return _lib.load()


# argument names in ABI order, and base values: N = 3025, F = 1870 is a split-F shape (ACM) whose workspace is missing
FWD = dict(X=PTR, x_dtype=0, ldx=1870, W=PTR, a1=PTR, a2=PTR, b1=PTR, b2=PTR, H=PTR, table_dtype=0, f1=PTR, f2=PTR,
           workspace=None, workspace_bytes=0, N=3025, F=1870, K=8, FP=8, in_drop=0.0, fts_drop=0.0, seed=0,
           seed_dev=None, row_offset=0, keep=None, flags=0, stream=None)
MULTI = dict(X=PTR, x_dtype=0, ldx=1870, W=PTR, a1=PTR, a2=PTR, b1=PTR, b2=PTR, H=PTR, table_dtype=0, f1=PTR, f2=PTR,
             workspace=None, workspace_bytes=0, N=3025, F=1870, K=8, FP=8, P=3, in_drop=0.0, fts_drop=0.0, seeds=None,
             seed_dev=None, row_offset=0, keep=None, flags=0, stream=None)
BWD = dict(X=PTR, x_dtype=0, ldx=1870, dH=PTR, dW=PTR, workspace=PTR, workspace_bytes=0, N=3025, F=1870, K=8, FP=8,
           in_drop=0.0, seed=0, seed_dev=None, row_offset=0, keep=None, stream=None)
BWD_IN = dict(dH=PTR, W=PTR, dX=PTR, ldo=1869, N=3025, F=1870, K=8, FP=8, in_drop=0.0, seed=0, seed_dev=None,
              row_offset=0, stream=None)
CLS = dict(Z=PTR, Wc=PTR, bc=PTR, labels=PTR, mask=PTR, row_weight=1.0, logits=PTR, loss_acc=PTR, dZ=None, dWc=None,
           dbc=None, workspace=PTR, workspace_bytes=0, N=100, D=64, C=3, HC=1, stream=None)
CLS_BWD = dict(Z=PTR, Wc=PTR, bc=PTR, dlogits=PTR, dZ=PTR, dWc=PTR, dbc=PTR, workspace=PTR, workspace_bytes=0, N=100,
               D=64, C=3, HC=1, stream=None)
BASE = {"han_project_fwd": FWD, "han_project_fwd_multi": MULTI, "han_project_bwd": BWD,
        "han_project_bwd_input": BWD_IN, "han_classifier_loss": CLS, "han_classifier_bwd": CLS_BWD}
PIPE = dict(N=40000, F=64, ldx=64)       # whole-F blocks of 128 rows: the matrix-pipe and fused-launch shape

CASES = [
    # --- han_project_fwd
    ("han_project_fwd", "n0_null_x", dict(N=0, X=None), 0),
    ("han_project_fwd", "n0_before_every_other_check", dict(N=0, X=None, K=8, FP=4, x_dtype=7, in_drop=1.0), 0),
    ("han_project_fwd", "null_x", dict(X=None), BADARG),
    ("han_project_fwd", "null_f2", dict(f2=None), BADARG),
    ("han_project_fwd", "negative_n", dict(N=-1), BADARG),
    ("han_project_fwd", "ldx_below_f", dict(ldx=1869), BADARG),
    ("han_project_fwd", "null_before_heads", dict(X=None, K=8, FP=4), BADARG),
    ("han_project_fwd", "heads_8x4", dict(K=8, FP=4), UNSUPPORTED),
    ("han_project_fwd", "x_dtype_7", dict(x_dtype=7), UNSUPPORTED),
    ("han_project_fwd", "table_dtype_7", dict(table_dtype=7), UNSUPPORTED),
    ("han_project_fwd", "dtype_before_dropout", dict(x_dtype=7, in_drop=1.0), UNSUPPORTED),
    ("han_project_fwd", "in_drop_1", dict(in_drop=1.0), BADARG),
    ("han_project_fwd", "fts_drop_negative", dict(fts_drop=-0.5), BADARG),
    ("han_project_fwd", "both_pipe_flags", dict(flags=EXACT_PIPE | MATRIX_PIPE), BADARG),
    ("han_project_fwd", "split_no_workspace", dict(), WORKSPACE),
    ("han_project_fwd", "split_workspace_too_small", dict(workspace=PTR, workspace_bytes=1000), WORKSPACE),
    ("han_project_fwd", "split_workspace_before_keep", dict(in_drop=0.5, keep=PTR), WORKSPACE),
    ("han_project_fwd", "keep_where_no_kernel_writes_one", dict(in_drop=0.5, keep=PTR, workspace=PTR, workspace_bytes=AMPLE), BADARG),
    ("han_project_fwd", "keep_without_dropout_is_ignored", dict(keep=PTR), WORKSPACE),
    ("han_project_fwd", "keep_on_the_exact_pipe", dict(PIPE, in_drop=0.5, keep=PTR, flags=EXACT_PIPE), BADARG),
    ("han_project_fwd", "keep_below_the_table_bound", dict(PIPE, N=20000, in_drop=0.5, keep=PTR, workspace=PTR, workspace_bytes=AMPLE), BADARG),
    ("han_project_fwd", "pipe_no_workspace", dict(PIPE, in_drop=0.5), WORKSPACE),
    ("han_project_fwd", "pipe_eval_on_request_no_workspace", dict(PIPE, flags=MATRIX_PIPE), WORKSPACE),
    ("han_project_fwd", "pipe_bf16_no_workspace", dict(PIPE, x_dtype=1), WORKSPACE),
    ("han_project_fwd", "pipe_workspace_too_small", dict(PIPE, in_drop=0.5, workspace=PTR, workspace_bytes=64), WORKSPACE),
    # --- han_project_fwd_multi
    ("han_project_fwd_multi", "p0", dict(P=0), BADARG),
    ("han_project_fwd_multi", "p0_before_n0", dict(P=0, N=0), BADARG),
    ("han_project_fwd_multi", "dropout_without_seeds", dict(in_drop=0.5), BADARG),
    ("han_project_fwd_multi", "dropout_without_seeds_before_n0", dict(in_drop=0.5, N=0, X=None), BADARG),
    ("han_project_fwd_multi", "n0_null_x", dict(N=0, X=None), 0),
    ("han_project_fwd_multi", "n0_before_dtype", dict(N=0, x_dtype=7), 0),
    ("han_project_fwd_multi", "null_x", dict(X=None), BADARG),
    ("han_project_fwd_multi", "heads_8x4", dict(K=8, FP=4), UNSUPPORTED),
    ("han_project_fwd_multi", "x_dtype_7", dict(x_dtype=7), UNSUPPORTED),
    ("han_project_fwd_multi", "table_dtype_7", dict(table_dtype=7), UNSUPPORTED),
    ("han_project_fwd_multi", "x_dtype_7_on_the_fused_shape", dict(PIPE, x_dtype=7, workspace=PTR, workspace_bytes=AMPLE), UNSUPPORTED),
    ("han_project_fwd_multi", "table_dtype_7_on_the_fused_shape", dict(PIPE, table_dtype=7, workspace=PTR, workspace_bytes=AMPLE), UNSUPPORTED),
    ("han_project_fwd_multi", "split_no_workspace", dict(), WORKSPACE),
    ("han_project_fwd_multi", "fused_no_workspace", dict(PIPE), WORKSPACE),
    ("han_project_fwd_multi", "fused_workspace_of_one_meta_path", dict(PIPE, workspace=PTR, workspace_bytes=ONE_IMAGE), WORKSPACE),
    ("han_project_fwd_multi", "fused_with_matrix_pipe_flag", dict(PIPE, flags=MATRIX_PIPE), WORKSPACE),
    ("han_project_fwd_multi", "both_pipe_flags_reach_the_single_call", dict(flags=EXACT_PIPE | MATRIX_PIPE), BADARG),
    # --- han_project_bwd
    ("han_project_bwd", "null_workspace", dict(workspace=None), BADARG),
    ("han_project_bwd", "null_workspace_before_dtype", dict(workspace=None, x_dtype=7), BADARG),
    ("han_project_bwd", "null_dh", dict(dH=None), BADARG),
    ("han_project_bwd", "ldx_below_f", dict(ldx=1869), BADARG),
    ("han_project_bwd", "heads_8x4", dict(K=8, FP=4), UNSUPPORTED),
    ("han_project_bwd", "x_dtype_7", dict(x_dtype=7), UNSUPPORTED),
    ("han_project_bwd", "dtype_before_dropout", dict(x_dtype=7, in_drop=1.0), UNSUPPORTED),
    ("han_project_bwd", "in_drop_1", dict(in_drop=1.0), BADARG),
    ("han_project_bwd", "dropout_before_workspace", dict(in_drop=-0.1, workspace_bytes=0), BADARG),
    ("han_project_bwd", "workspace_too_small", dict(workspace_bytes=1000), WORKSPACE),
    ("han_project_bwd", "workspace_before_keep", dict(in_drop=0.5, keep=PTR), WORKSPACE),
    ("han_project_bwd", "keep_on_a_shape_without_a_table", dict(in_drop=0.5, keep=PTR, workspace_bytes=AMPLE), BADARG),
    ("han_project_bwd", "keep_below_the_table_bound", dict(PIPE, N=32767, in_drop=0.5, keep=PTR, workspace_bytes=AMPLE), BADARG),
    ("han_project_bwd", "keep_misaligned", dict(PIPE, in_drop=0.5, keep=PTR + 4, workspace_bytes=AMPLE), BADARG),
    ("han_project_bwd", "keep_with_unaligned_x", dict(PIPE, X=PTR + 4, in_drop=0.5, keep=PTR, workspace_bytes=AMPLE), BADARG),
    ("han_project_bwd", "keep_with_other_heads", dict(PIPE, K=4, FP=16, in_drop=0.5, keep=PTR, workspace_bytes=AMPLE), BADARG),
    # --- han_project_bwd_input
    ("han_project_bwd_input", "ldo_below_f", dict(), BADARG),
    ("han_project_bwd_input", "null_dh", dict(dH=None, ldo=1870), BADARG),
    ("han_project_bwd_input", "null_before_n0", dict(dX=None, ldo=1870, N=0), BADARG),
    ("han_project_bwd_input", "negative_n", dict(ldo=1870, N=-1), BADARG),
    ("han_project_bwd_input", "heads_8x4", dict(ldo=1870, K=8, FP=4), UNSUPPORTED),
    ("han_project_bwd_input", "heads_before_dropout", dict(ldo=1870, K=3, FP=8, in_drop=1.0), UNSUPPORTED),
    ("han_project_bwd_input", "in_drop_1", dict(ldo=1870, in_drop=1.0), BADARG),
    ("han_project_bwd_input", "dropout_before_n0", dict(ldo=1870, in_drop=1.0, N=0), BADARG),
    ("han_project_bwd_input", "n0", dict(ldo=1870, N=0), 0),
    # --- han_classifier_loss
    ("han_classifier_loss", "d64_no_workspace_bytes", dict(), WORKSPACE),
    ("han_classifier_loss", "d65", dict(D=65), UNSUPPORTED),
    ("han_classifier_loss", "d0", dict(D=0), UNSUPPORTED),
    ("han_classifier_loss", "c0", dict(C=0), UNSUPPORTED),
    ("han_classifier_loss", "shape_before_workspace_bytes", dict(D=65, workspace_bytes=AMPLE), UNSUPPORTED),
    ("han_classifier_loss", "null_z", dict(Z=None), BADARG),
    ("han_classifier_loss", "null_workspace_before_shape", dict(workspace=None, D=65), BADARG),
    ("han_classifier_loss", "hc0", dict(HC=0), BADARG),
    ("han_classifier_loss", "negative_n", dict(N=-1), BADARG),
    ("han_classifier_loss", "backward_without_dwc", dict(dZ=PTR, dbc=PTR), BADARG),
    ("han_classifier_loss", "backward_without_dbc", dict(dZ=PTR, dWc=PTR, workspace_bytes=AMPLE), BADARG),
    ("han_classifier_loss", "shape_before_backward_pointers", dict(dZ=PTR, D=65), UNSUPPORTED),
    ("han_classifier_loss", "wide_no_workspace_bytes", dict(D=128, C=40), WORKSPACE),
    ("han_classifier_loss", "general_no_workspace_bytes", dict(D=192, C=3), WORKSPACE),
    ("han_classifier_loss", "general_many_classes_small_workspace", dict(D=64, C=65, workspace_bytes=4096), WORKSPACE),
    # --- han_classifier_bwd
    ("han_classifier_bwd", "no_workspace_bytes", dict(), WORKSPACE),
    ("han_classifier_bwd", "workspace_of_the_means_only", dict(workspace_bytes=(64 * 3 + 3) * 4), WORKSPACE),
    ("han_classifier_bwd", "d65", dict(D=65), UNSUPPORTED),
    ("han_classifier_bwd", "c0", dict(C=0, workspace_bytes=AMPLE), UNSUPPORTED),
    ("han_classifier_bwd", "null_dlogits", dict(dlogits=None), BADARG),
    ("han_classifier_bwd", "null_workspace_before_shape", dict(workspace=None, D=65), BADARG),
    ("han_classifier_bwd", "hc0", dict(HC=0), BADARG),
    ("han_classifier_bwd", "negative_n", dict(N=-1), BADARG),
]


@pytest.mark.parametrize("fn,name,over,want", CASES, ids=[f"{c[0][4:]}-{c[1]}" for c in CASES])
def test_validation_returns_before_any_launch(lib, fn, name, over, want):
    args = dict(BASE[fn])
    assert set(over) <= set(args), "a case overrides named arguments only"
    args.update(over)
    if callable(args.get("workspace_bytes")):
        args["workspace_bytes"] = args["workspace_bytes"](lib)
        assert 0 < args["workspace_bytes"] < lib.han_project_fwd_multi_workspace(args["N"], args["F"], 8, 8, args["P"])
    assert getattr(lib, fn)(*args.values()) == want


def test_case_ids_are_unique_and_every_entry_point_is_covered():
    assert len({(c[0], c[1]) for c in CASES}) == len(CASES)
    assert {c[0] for c in CASES} == set(BASE)
