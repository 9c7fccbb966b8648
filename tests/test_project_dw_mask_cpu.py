"""The scalar keep-word loads of dW (project_bwd_blk_kernel) have no range check: the last byte they may touch,
from the same arithmetic the kernel addresses with (han_project_bwd_keep_last_byte), must lie inside the table that
han_project_keep_bytes() makes the caller allocate.  Host-side queries only: no GPU."""
from han_amd import _lib

FS = range(8, 513, 8)
NS = list(range(32768, 32768 + 131)) + [1_000_000, 1_000_001, (1 << 31) - 1, 1 << 31, (1 << 32) + 5, (1 << 40) + 33]


def test_last_byte_touched_lies_inside_the_table():
    lib = _lib.load()
    for n in NS:
        for f in FS:
            size = int(lib.han_project_keep_bytes(n, f, f, 8, 8))
            last = int(lib.han_project_bwd_keep_last_byte(n, f))
            assert size == n * f + 128, (n, f, size)
            # the farthest wave: row n - 1, the last 128-feature block, wave 3, 32 bytes
            assert last == (n - 1) * f + (f - 1) // 128 * 128 + 96 + 31, (n, f, last)
            assert n * f <= last + 128 and last < size, (n, f, last, size)


def test_last_byte_reaches_the_slack_bound_at_one_octet():
    lib = _lib.load()
    for f in (8, 136, 264):      # a last feature block of 8 features: the worst case, 8 bytes below the slack's end
        assert int(lib.han_project_bwd_keep_last_byte(32768, f)) == 32768 * f + 119


def test_no_rows_no_bytes():
    lib = _lib.load()
    assert int(lib.han_project_bwd_keep_last_byte(0, 8)) == -1
