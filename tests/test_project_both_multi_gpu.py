"""han_project_fwd_both with more than two meta-paths: ONE launch of the combined kernel serves up to 8 of them.

A block finds its (row tile, meta-path) from its block id alone -- tile 8 (r / P) + b % 8 of meta-path r % P, r = b / 8 --
so the shapes are the ones at which that map can go wrong: tile counts that are no multiple of 8 (257 tiles with a
partial last tile of 72 rows, and 263 whole tiles), P = 4 and 6 (6 does not divide the 8 blocks of a round), and P = 10,
which takes two launches (8 + 2 meta-paths).  F = 8 is a lone partial K-step, F = 136 one full keep-line flush plus a
partial group.  Both row sets and the keep tables must carry the BYTES of the separate calls, as at P = 2
(test_project_both_gpu.py)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

ROW_OFFSETS = (0, 1_000_003)


def _bits(t):
    return t.view(torch.uint8) if t.dtype == torch.uint8 else t.contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


_inputs = {}


def _case(dev, n, f, p):
    """X, the parameters and the eval reference of one shape, made once and never written again."""
    key = (n, f, p)
    if key not in _inputs:
        from han_amd import ops
        g = torch.Generator(device=dev).manual_seed(1000 * f + n % 1000 + p)
        rnd = lambda *s: torch.randn(s, device=dev, generator=g)
        prm = (rnd(p, f, 64) * 0.1, rnd(p, 8, 8), rnd(p, 8, 8), rnd(p, 8), rnd(p, 8))
        X = rnd(n, f)
        _inputs[key] = (X, prm, ops.project_fwd_multi(X, *prm))
    return _inputs[key]


def _check(dev, n, f, p, drops, ro):
    from han_amd import ops
    X, prm, ev_ref = _case(dev, n, f, p)
    seeds = [0x1234567 + 0x9E3779B97F4A7C15 * i for i in range(p)]
    got = ops.project_fwd_both(X, *prm, drops[0], drops[1], seeds, row_offset=ro)
    assert got is not None, "eligible shape declined"
    (H, f1, f2, keep), (He, f1e, f2e) = got
    rH, rf1, rf2, rkeep = ops.project_fwd_multi(X, *prm, in_drop=drops[0], fts_drop=drops[1], seeds=seeds,
                                                row_offset=ro, want_keep=True)
    for q in range(p):      # per meta-path, so that a failure names the one that went to the wrong block
        what = f"meta-path {q} of {p}, row_offset={ro}"
        assert _same(H[q], rH[q]), f"training H differs ({what})"
        assert _same(f1[q], rf1[q]) and _same(f2[q], rf2[q]), f"training scores differ ({what})"
        # the last 128 bytes of a table are slack for whole-tile loads: never written
        assert _same(keep[q][:n * f], rkeep[q][:n * f]), f"keep table differs ({what})"
        assert _same(He[q], ev_ref[0][q]), f"eval H differs ({what})"
        assert _same(f1e[q], ev_ref[1][q]) and _same(f2e[q], ev_ref[2][q]), f"eval scores differ ({what})"


@pytest.mark.parametrize("drops", [(0.6, 0.6), (0.6, 0.0)], ids=["in06_fts06", "in06_fts0"])
@pytest.mark.parametrize("f", [8, 136])
@pytest.mark.parametrize("n", [32768 + 72, 33664], ids=["257tiles_partial", "263tiles"])
@pytest.mark.parametrize("p", [4, 6])
def test_one_launch_for_all_meta_paths_carries_the_bytes_of_the_separate_calls(dev, p, n, f, drops):
    for ro in ROW_OFFSETS:
        _check(dev, n, f, p, drops, ro)


def test_ten_meta_paths_run_as_a_group_of_eight_and_a_group_of_two(dev):
    _check(dev, 32768 + 72, 8, 10, (0.6, 0.6), 0)
