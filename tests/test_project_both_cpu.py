"""Host side of the shared projection: rng.peek_seeds, the stash key and its take / drop rules, and what
han_project_fwd_both decides before any launch (dummy pointers, as in test_return_codes_cpu.py: no launch is reached)."""
import ctypes
import types

import pytest
import torch

from han_amd import rng

BADARG, UNSUPPORTED, WORKSPACE, NOT_ELIGIBLE = -1, -2, -3, -4
PTR = 0x10000          # non-null, 16-byte aligned, never dereferenced


def test_peek_seeds_are_the_next_seeds_and_leave_the_counter():
    saved = dict(rng._state)
    try:
        rng.manual_seed(77)
        for _ in range(3):
            rng.next_seed()
        before = dict(rng._state)
        peek = rng.peek_seeds(5)
        assert rng._state == before and rng.peek_seeds(5) == peek and rng.peek_seeds(2) == peek[:2]
        assert rng.peek_seeds(0) == ()
        assert tuple(rng.next_seed() for _ in range(5)) == peek
        assert rng.peek_seeds(1) != peek[4:5]
    finally:
        rng._state.update(saved)


def test_stash_key_follows_step_version_and_address():
    from han_amd import layers
    flat = torch.zeros(16)
    k0 = layers.stash_key(3, flat)
    assert k0 == layers.stash_key(3, flat)
    assert layers.stash_key(4, flat) != k0                      # the native Adam step: counted, not versioned
    flat[2:4].view(2).copy_(torch.ones(2))                      # a torch-side write through a view
    assert layers.stash_key(3, flat) != k0
    assert layers.stash_key(3, flat.clone()) != layers.stash_key(3, flat)


def test_a_stash_is_taken_once_and_only_for_the_projection_it_was_made_for():
    from han_amd import layers
    flat, opt = torch.zeros(8), types.SimpleNamespace(t=5)
    sp = layers.SharedProjection(lambda: flat, lambda: opt.t)
    X, tables = torch.zeros(4, 4), ("H", "f1", "f2", ["k"])

    def put():
        sp._stash = (sp.key(), X, 0.6, (11, 12), 0, torch.float32, tables)
    put()
    assert sp.take(X, 0.6, [11, 12], 0, torch.float32) is tables and sp.taken == 1
    assert sp.take(X, 0.6, [11, 12], 0, torch.float32) is None                      # consumed
    for bad in ((X.clone(), 0.6, (11, 12), 0, torch.float32), (X, 0.5, (11, 12), 0, torch.float32),
                (X, 0.6, (11, 13), 0, torch.float32), (X, 0.6, (11, 12), 1, torch.float32),
                (X, 0.6, (11, 12), 0, torch.bfloat16)):
        put()
        assert sp.take(*bad) is None and sp._stash is None                          # not taken: freed
    put(); opt.t = 6
    assert sp.take(X, 0.6, (11, 12), 0, torch.float32) is None
    put(); flat.add_(1.0)
    assert sp.take(X, 0.6, (11, 12), 0, torch.float32) is None
    put(); sp.drop()
    assert sp.take(X, 0.6, (11, 12), 0, torch.float32) is None and sp.taken == 1
    assert layers.SharedProjection.stash_bytes(1_000_000, 256, 4) == 4 * (256_000_000 + 64_000_000 + 256_000_000 + 128)


@pytest.fixture(scope="module")
def lib():
    if torch.cuda.is_available():
        pytest.skip("dummy pointers: only where no launch can start")
    from han_amd import _lib
    _lib.build()
    return _lib.load()


NAMES = ("X x_dtype ldx W a1 a2 b1 b2 H table_dtype f1 f2 H_eval f1_eval f2_eval workspace workspace_bytes N F K FP P "
         "in_drop fts_drop seeds seed_dev row_offset keep flags stream").split()
SEEDS = (ctypes.c_uint64 * 4)(1, 2, 3, 4)
# an eligible call (the first row count with a keep table) that ends at the missing workspace, before any launch
BASE = dict(X=PTR, x_dtype=0, ldx=64, W=PTR, a1=PTR, a2=PTR, b1=PTR, b2=PTR, H=PTR, table_dtype=0, f1=PTR, f2=PTR,
            H_eval=PTR, f1_eval=PTR, f2_eval=PTR, workspace=None, workspace_bytes=0, N=32768, F=64, K=8, FP=8, P=2,
            in_drop=0.6, fts_drop=0.6, seeds=SEEDS, seed_dev=None, row_offset=0, keep=PTR, flags=0, stream=None)
CASES = [
    ("eligible_no_workspace", dict(), WORKSPACE),
    ("eligible_workspace_too_small", dict(workspace=PTR, workspace_bytes=2 * 2 * 12288 - 1), WORKSPACE),
    ("p0", dict(P=0), BADARG),
    ("dropout_without_seeds", dict(seeds=None), BADARG),
    ("dropout_without_seeds_before_n0", dict(seeds=None, N=0), BADARG),
    ("n0_null_x", dict(N=0, X=None), 0),
    ("null_x", dict(X=None), BADARG),
    ("null_eval_table", dict(H_eval=None), BADARG),
    ("null_eval_scores", dict(f2_eval=None), BADARG),
    ("ldx_below_f", dict(ldx=63), BADARG),
    ("null_before_heads", dict(f1_eval=None, K=8, FP=4), BADARG),
    ("heads_8x4", dict(K=8, FP=4), UNSUPPORTED),
    ("x_dtype_7", dict(x_dtype=7), UNSUPPORTED),
    ("dtype_before_dropout", dict(table_dtype=7, in_drop=1.0), UNSUPPORTED),
    ("in_drop_1", dict(in_drop=1.0), BADARG),
    ("both_pipe_flags", dict(flags=2 | 4), BADARG),
    ("bad_dropout_before_eligibility", dict(P=3, fts_drop=-0.5), BADARG),
    # valid calls outside the combined kernel's shapes
    ("odd_p", dict(P=3), NOT_ELIGIBLE),
    ("f_not_a_multiple_of_8", dict(F=12, ldx=12), NOT_ELIGIBLE),
    ("below_the_keep_table_bound", dict(N=32767), NOT_ELIGIBLE),
    ("no_keep_table", dict(keep=None), NOT_ELIGIBLE),
    ("no_input_dropout", dict(in_drop=0.0), NOT_ELIGIBLE),
    ("bf16_x", dict(x_dtype=1), NOT_ELIGIBLE),
    ("bf16_tables", dict(table_dtype=1), NOT_ELIGIBLE),
    ("exact_pipe", dict(flags=2), NOT_ELIGIBLE),
    ("four_wave_form", dict(flags=16), NOT_ELIGIBLE),
    ("unaligned_x", dict(X=PTR + 4), NOT_ELIGIBLE),
    ("ldx_not_a_multiple_of_4", dict(ldx=66), NOT_ELIGIBLE),
    ("not_eligible_before_workspace", dict(P=3, workspace=None), NOT_ELIGIBLE),
]


@pytest.mark.parametrize("name,over,want", CASES, ids=[c[0] for c in CASES])
def test_fwd_both_return_codes(lib, name, over, want):
    a = dict(BASE, **over)
    assert lib.han_project_fwd_both(*[a[n] for n in NAMES]) == want


def test_fwd_both_workspace_is_the_w_images_of_p_meta_paths(lib):
    for n, f, p in ((32768, 64, 2), (1_000_000, 256, 4), (40000, 40, 2)):
        assert lib.han_project_fwd_both_workspace(n, f, 8, 8, p) == ((f + 31) // 32) * p * 12288
        assert lib.han_project_fwd_both_workspace(n, f, 8, 8, p) == lib.han_project_fwd_multi_workspace(n, f, 8, 8, p)
    assert b"nothing was launched" in lib.han_error_string(NOT_ELIGIBLE)
