"""The silhouette kernel (han_silhouette in han_amd/csrc/evaluate.hip) and its Python layers against NumPy float64.

The reference and the rounding bound are tests/silhouette_ref.py: direct differences in float64, and a bound derived
from the fp32 pair bound of tests/test_evaluate_gpu.py (not measured).  A row whose max(a, b) is within twice its own
error is undecided and left out of the per-row comparison; every case asserts that at most 1 % of its rows are."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from han_amd import _lib, evaluate, ops
from tests import silhouette_ref as ref

pytestmark = pytest.mark.gpu

U = ref.U
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "exp_silhouette_ref.npz")


def _t(a, dev):
    return torch.tensor(np.ascontiguousarray(a)).to(dev)


def _sizes_64():
    """62 uneven clusters and two empty ones (5 and 63, the last), 4099 rows"""
    rs = np.random.RandomState(64)
    sizes = rs.randint(20, 100, size=64)
    sizes[[5, 63]] = 0
    sizes[10] += 4099 - sizes.sum()
    assert sizes.min() >= 0 and sizes[10] > 0 and sizes.sum() == 4099
    return sizes


# name -> (sizes, D, centre spread).  257: a tail tile, a width that is no multiple of 4; 1000: a cluster of one row,
# segments that straddle 64-row tiles, three 64-column stages; 37: less than one tile, one column split; 4099: 64
# clusters, two of them empty; 256: one column split (a and b are finished inside the tile kernel) with an empty
# cluster, a cluster of one row and a cluster of three column tiles
CASES = {
    "257x13": ((64, 65, 63, 65), 13, 3.0),
    "1000x130": ((1, 65, 934), 130, 1.0),
    "37x8": ((18, 19), 8, 3.0),
    "4099x64": (_sizes_64(), 64, 1.0),
    "256x70": ((130, 0, 1, 100, 25), 70, 1.0),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    sizes, dim, spread = CASES[name]
    x, codes, seg = ref.blobs(len(name) + dim, sizes, dim, spread)
    for a in (x, codes, seg):
        a.setflags(write=False)
    return x, codes, seg, ref.reference(x, codes, len(sizes))


@functools.lru_cache(maxsize=None)
def _result(name):
    x, _, seg, _ = _case(name)
    dev = torch.device("cuda:0")
    return ops.silhouette(_t(x, dev), _t(seg, dev))


def _check_rows(got, want, n_rows):
    """a, b, s of `got` (dict of tensors) against the reference dict, row by row within the derived bounds"""
    a, b, s = (got[key].cpu().numpy().astype(np.float64) for key in ("a", "b", "s"))
    assert a.shape == b.shape == s.shape == (n_rows,)
    und = want["undecided"]
    print("undecided %d of %d, max row bound %.3g, max |s - ref| %.3g" % (
        und.sum(), n_rows, want["bound"][~und].max(), np.abs(s - want["s"])[~und].max()))
    assert und.mean() <= 0.01
    assert (np.abs(a - want["a"]) <= want["e_a"]).all()
    assert (np.abs(b - want["b"]) <= want["e_b"]).all()
    assert (np.abs(s - want["s"])[~und] <= want["bound"][~und]).all()
    assert (np.abs(s) <= 1.0).all()
    return a, b, s


@pytest.mark.parametrize("name", list(CASES))
def test_rows_and_score_within_the_derived_bound(dev, name):
    x, codes, seg, want = _case(name)
    got = _result(name)
    n = x.shape[0]
    assert got["s"].dtype == torch.float32 and got["sum"].dtype == torch.float64
    a, b, s = _check_rows(got, want, n)
    single = np.diff(seg)[codes] == 1
    assert (s[single] == 0).all() and (a[single] == 0).all()          # a cluster of one row
    total = float(got["sum"].cpu()[0])
    assert total == pytest.approx(float(np.sum(got["s"].cpu().numpy().astype(np.float64))), abs=1e-9)
    assert abs(total / n - want["score"]) <= want["score_bound"]


def test_one_split_many_row_tiles_is_exact_on_a_line(dev):
    """33 000 rows: more than 512 row tiles, so the column range is not split and the tile kernel finishes a and b
    itself.  Integer points on a line (D = 1): every distance, every fp32 partial sum (< 2^24) and every double sum
    is an integer (coordinates below 2^11: |x_i|^2 + |x_j|^2 and 2 x_i x_j stay below 2^23), so S is exact and a, b
    are the correctly rounded quotients; the float64 reference costs O(N log N) (ref.line_sums)."""
    n, k = 33000, 3
    rs = np.random.RandomState(33)
    codes = np.sort(rs.randint(0, k, n))
    v = rs.randint(0, 2048, n)
    counts = np.bincount(codes, minlength=k)
    seg = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    S = ref.line_sums(v, codes, k).astype(np.float64)
    rows = np.arange(n)
    a = S[rows, codes] / (counts[codes] - 1)
    b = np.where(np.arange(k)[None, :] != codes[:, None], S / counts[None, :], np.inf).min(1)
    s = (b - a) / np.maximum(a, b)
    got = ops.silhouette(_t(v.astype(np.float32), dev).reshape(n, 1), _t(seg, dev))
    np.testing.assert_array_equal(got["a"].cpu().numpy(), a.astype(np.float32))
    np.testing.assert_array_equal(got["b"].cpu().numpy(), b.astype(np.float32))
    np.testing.assert_array_equal(got["s"].cpu().numpy(), s.astype(np.float32))
    assert float(got["sum"].cpu()[0]) == pytest.approx(float(s.astype(np.float32).astype(np.float64).sum()), abs=1e-7)


def test_cluster_of_bit_identical_rows(dev):
    """70 copies of one row as a cluster of their own: a is within its bound of 0, s within its bound of 1"""
    x, codes, seg = ref.blobs(7, (70, 90, 40), 13, 3.0)
    x[:70] = x[0]
    want = ref.reference(x, codes, 3)
    assert (want["a"][:70] == 0).all() and (want["s"][:70] == 1).all() and not want["undecided"].any()
    got = ops.silhouette(_t(x, dev), _t(seg, dev))
    a, _, s = _check_rows(got, want, 200)
    assert (a[:70] <= want["e_a"][:70]).all() and (1 - s[:70] <= want["bound"][:70]).all()


def test_strided_rows_and_two_runs_are_bitwise_equal(dev):
    x, _, seg, _ = _case("257x13")
    big = np.zeros((257, 24), dtype=np.float32)
    big[:, 3:16] = x
    big[:, 16:] = 99.0
    view = _t(big, dev)[:, 3:16]
    assert view.stride(0) == 24
    strided = ops.silhouette(view, _t(seg, dev))
    for name, other in (("257x13", strided), ("4099x64", None), ("37x8", None)):
        xc, _, sc, _ = _case(name)
        first = _result(name)
        again = other if other is not None else ops.silhouette(_t(xc, dev), _t(sc, dev))
        for key in ("a", "b", "s", "sum"):
            assert torch.equal(first[key], again[key]), (name, key)


def test_samples_return_in_the_callers_order_for_any_integer_labels(dev):
    x, codes, seg, want = _case("257x13")
    perm = np.random.RandomState(2).permutation(257)
    names = np.array([-7, 3, 1000, 4])                      # sorted: -7, 3, 4, 1000 -> codes 0, 1, 3, 2
    xs, labels = x[perm], names[codes][perm]
    got = evaluate.silhouette_samples(_t(xs, dev), _t(labels, dev))
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (257,)
    uniq, inv = np.unique(labels, return_inverse=True)
    order = np.argsort(inv, kind="stable")
    seg2 = np.concatenate([[0], np.cumsum(np.bincount(inv))]).astype(np.int64)
    grouped = ops.silhouette(_t(xs[order], dev), _t(seg2, dev))
    assert torch.equal(got[_t(order, dev)], grouped["s"])             # element for element
    und = want["undecided"][perm]
    assert (np.abs(got.cpu().numpy() - want["s"][perm])[~und] <= want["bound"][perm][~und]).all()
    assert torch.equal(evaluate.silhouette_samples(xs, labels, device=dev), got)      # NumPy in, device asked for
    score = evaluate.silhouette_score(_t(xs, dev), labels)
    assert isinstance(score, float) and abs(score - want["score"]) <= want["score_bound"]


def test_sample_size_takes_the_permutation_prefix(dev):
    x, codes, _, want = _case("257x13")
    idx = np.random.RandomState(5).permutation(257)[:100]
    sub = evaluate.silhouette_score(_t(x, dev), _t(codes, dev), sample_size=100, seed=5)
    assert sub == evaluate.silhouette_score(_t(x[idx], dev), _t(codes[idx], dev))
    want_sub = ref.reference(x[idx], codes[idx], 4)
    assert not want_sub["undecided"].any()
    assert abs(sub - want_sub["score"]) <= want_sub["score_bound"]
    assert abs(sub - want["score"]) > want_sub["score_bound"] + want["score_bound"]      # not the full score


def test_fixture_rows_against_scikit_learn_float64(dev):
    f = np.load(GOLDEN)
    x, labels = f["x"], f["labels"]
    want = ref.reference(x, labels, 4)
    assert np.abs(want["s"] - f["samples"]).max() <= 1e-12             # the NumPy reference is scikit-learn's
    assert not want["undecided"].any()
    got = evaluate.silhouette_samples(x, labels, device=dev).cpu().numpy().astype(np.float64)
    assert (np.abs(got - f["samples"]) <= want["bound"] + 1e-12).all()
    score = evaluate.silhouette_score(x, labels, device=dev)
    assert abs(score - f["samples"].mean()) <= want["score_bound"]


def test_my_kmeans_reports_the_silhouette_of_its_own_fits(dev, capsys):
    f = np.load(GOLDEN)
    x, y = f["x"], f["y"]
    three = evaluate.my_Kmeans(x, y, k=4, time=3, seed=0, device=dev, silhouette=True)
    line = capsys.readouterr().out.strip().splitlines()[-1]
    assert line == "NMI (10 avg): {:.4f} , ARI (10avg): {:.4f}, silhouette(10avg): {:.4f}".format(*three)
    two = evaluate.my_Kmeans(x, y, k=4, time=3, seed=0, device=dev, verbose=False)
    assert len(three) == 3 and all(isinstance(v, float) for v in three)
    assert len(two) == 2 and three[:2] == two                           # bit for bit: no extra draws
    rs = np.random.RandomState(0)
    scores, bounds = [], []
    for _ in range(3):
        labels = evaluate.kmeans(x, 4, seed=rs, device=dev)["labels"].cpu().numpy()
        codes = np.unique(labels, return_inverse=True)[1]
        want = ref.reference(x, codes)
        assert not want["undecided"].any()
        scores.append(want["score"])
        bounds.append(want["score_bound"])
    assert abs(three[2] - np.mean(scores)) <= np.mean(bounds)


def test_errors(dev):
    x, codes, seg, _ = _case("37x8")
    xt = _t(x, dev)
    rs = np.random.RandomState(1)
    for bad in (np.zeros(37, dtype=np.int64), np.arange(37)):           # one label, n labels
        with pytest.raises(ValueError, match="Number of labels"):
            evaluate.silhouette_samples(xt, bad)
    wide = _t(rs.standard_normal((130, 4)).astype(np.float32), dev)
    with pytest.raises(ValueError, match="at most 64"):
        evaluate.silhouette_samples(wide, np.arange(130) % 65)
    with pytest.raises(ValueError, match="at most 512"):
        evaluate.silhouette_score(_t(rs.standard_normal((37, 513)).astype(np.float32), dev), codes)
    with pytest.raises(ValueError):
        ops.silhouette(wide, _t(np.linspace(0, 130, 67).astype(np.int64), dev))      # k = 66
    with pytest.raises(ValueError):
        ops.silhouette(xt.cpu(), _t(seg, dev))
    lib = _lib.load()
    total = torch.zeros(1, dtype=torch.float64, device=dev)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
    seg65 = _t(np.arange(66, dtype=np.int64), dev)
    args = (None, None, None, total.data_ptr(), ws.data_ptr(), ws.numel(), None)
    assert lib.han_silhouette(wide.data_ptr(), 4, seg65.data_ptr(), 65, 4, 65, *args) == -2       # HAN_E_UNSUPPORTED
    assert lib.han_silhouette(None, 8, _t(seg, dev).data_ptr(), 37, 8, 2, *args) == -1            # HAN_E_BADARG
    assert lib.han_silhouette(xt.data_ptr(), 8, _t(seg, dev).data_ptr(), 37, 8, 2, None, None, None, total.data_ptr(),
                              ws.data_ptr(), 16, None) == -3                                      # HAN_E_WORKSPACE
    total.fill_(7.0)
    assert lib.han_silhouette(None, 8, None, 0, 8, 2, *args) == 0                                 # N = 0
    torch.cuda.synchronize()
    assert float(total.cpu()[0]) == 0.0
