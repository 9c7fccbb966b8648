"""What han_node_attn_bwd_cols_scores decides before any launch (dummy pointers, as in test_return_codes_cpu.py: no
launch is reached): the workspace query, the order of the checks, and the calls it declines with HAN_E_NOT_ELIGIBLE."""
import ctypes

import pytest
import torch

BADARG, UNSUPPORTED, WORKSPACE, NOT_ELIGIBLE = -1, -2, -3, -4
PTR = 0x10000          # non-null, 16-byte aligned, never dereferenced
FLAG_MASKED_EDGES, FLAG_LEAN = 64, 256


@pytest.fixture(scope="module")
def lib():
    if torch.cuda.is_available():
        pytest.skip("dummy pointers: only where no launch can start")
    from han_amd import _lib
    _lib.build()
    return _lib.load()


NAMES = ("colptr rowidx edge_val gs table_gid H table_dtype f2 df1 a1 a2 dH df2 NS E K FP slope coef_drop fts_drop seed "
         "seed_dev src_offset dst_offset flags split dense da1 da2 db1 db2 workspace workspace_bytes stream").split()
# every case ends before a launch: the base call at the workspace that is too small by one byte
BASE = dict(colptr=PTR, rowidx=PTR, edge_val=None, gs=PTR, table_gid=None, H=PTR, table_dtype=0, f2=PTR, df1=PTR, a1=PTR,
            a2=PTR, dH=PTR, df2=PTR, NS=1000, E=5000, K=8, FP=8, slope=0.2, coef_drop=0.6, fts_drop=0.6, seed=3,
            seed_dev=None, src_offset=0, dst_offset=0, flags=0, split=None, dense=None, da1=PTR, da2=PTR, db1=PTR, db2=PTR,
            workspace=PTR, workspace_bytes=0, stream=None)


def _split(**kw):
    from han_amd import _lib
    f = dict(split_deg=1024, n_long=0, n_chunks=0, long_rows=None, long_ptr=None, chunk_long=None, chunk_start=None,
             chunk_end=None, workspace=None, workspace_bytes=0, n_short=0, n_mid=0, short_rows=None, mid_rows=None)
    f.update(kw)
    return _lib.HanRowSplit(*[f[n] for n, _ in _lib.HanRowSplit._fields_])


def _dense():
    from han_amd import _lib
    return _lib.HanDense(PTR, 16, 1000, PTR, 1 << 20)


def _call(lib, over, enough=True):
    a = dict(BASE, **over)
    if enough and "workspace_bytes" not in over:
        a["workspace_bytes"] = lib.han_node_attn_bwd_cols_scores_workspace(a["NS"], a["K"], a["FP"])
    keep = [a["split"], a["dense"]]
    a["split"] = ctypes.byref(keep[0]) if keep[0] is not None else None
    a["dense"] = ctypes.byref(keep[1]) if keep[1] is not None else None
    return lib.han_node_attn_bwd_cols_scores(*[a[n] for n in NAMES])


def test_workspace_is_two_launches_of_slab_rows_and_the_fold(lib):
    for k, fp in ((8, 8), (4, 16), (1, 64)):
        assert lib.han_node_attn_bwd_cols_scores_workspace(1_000_000, k, fp) == (2 * 8192 + 256) * (128 + 2 * k) * 4
        assert lib.han_node_attn_bwd_cols_scores_workspace(10, k, fp) == lib.han_node_attn_bwd_cols_scores_workspace(1 << 30, k, fp)
    assert b"nothing was launched" in lib.han_error_string(NOT_ELIGIBLE)


CASES = [
    # argument checks, in their order
    ("null_colptr", lambda: dict(colptr=None), BADARG),
    ("null_rowidx_with_entries", lambda: dict(rowidx=None), BADARG),
    ("null_df1", lambda: dict(df1=None), BADARG),
    ("null_da1", lambda: dict(da1=None), BADARG),
    ("null_db2", lambda: dict(db2=None), BADARG),
    ("null_workspace", lambda: dict(workspace=None), BADARG),
    ("negative_ns", lambda: dict(NS=-1), BADARG),
    ("bins_beyond_the_rows", lambda: dict(split=_split(n_short=900, n_mid=200, short_rows=PTR, mid_rows=PTR)), BADARG),
    ("null_before_heads", lambda: dict(da2=None, K=8, FP=4), BADARG),
    ("heads_8x4", lambda: dict(K=8, FP=4), UNSUPPORTED),
    ("table_dtype_7", lambda: dict(table_dtype=7), UNSUPPORTED),
    ("dtype_before_dropout", lambda: dict(table_dtype=7, coef_drop=1.0), UNSUPPORTED),
    ("coef_drop_1", lambda: dict(coef_drop=1.0), BADARG),
    ("fts_drop_negative", lambda: dict(fts_drop=-0.5), BADARG),
    ("bad_dropout_before_workspace", lambda: dict(fts_drop=1.0, workspace_bytes=0), BADARG),
    ("workspace_one_byte_short", lambda: dict(workspace_bytes=(2 * 8192 + 256) * 144 * 4 - 1), WORKSPACE),
    ("workspace_before_eligibility", lambda: dict(workspace_bytes=0, flags=FLAG_LEAN), WORKSPACE),
    # valid calls the combined kernels do not take
    ("no_rows", lambda: dict(NS=0, E=0), NOT_ELIGIBLE),
    ("lean", lambda: dict(flags=FLAG_LEAN), NOT_ELIGIBLE),
    ("masked_backward", lambda: dict(flags=FLAG_MASKED_EDGES), NOT_ELIGIBLE),
    ("dense_bit_mask", lambda: dict(flags=FLAG_LEAN, dense=_dense()), NOT_ELIGIBLE),
    ("dense_bit_mask_without_lean", lambda: dict(dense=_dense()), NOT_ELIGIBLE),
    ("long_rows", lambda: dict(split=_split(n_long=1, n_chunks=2, long_rows=PTR, long_ptr=PTR, chunk_long=PTR, chunk_start=PTR,
                                            chunk_end=PTR, workspace=PTR, workspace_bytes=1 << 20, n_short=999,
                                            short_rows=PTR)), NOT_ELIGIBLE),
    ("bins_that_leave_rows_out", lambda: dict(split=_split(n_short=600, n_mid=300, short_rows=PTR, mid_rows=PTR)), NOT_ELIGIBLE),
]


@pytest.mark.parametrize("name,over,want", CASES, ids=[c[0] for c in CASES])
def test_bwd_cols_scores_return_codes(lib, name, over, want):
    assert _call(lib, over()) == want
