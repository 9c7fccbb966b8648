"""The evaluation kernels (han_amd/csrc/evaluate.hip) against NumPy: brute-force k nearest neighbours, the vote,
contingency tables, one Lloyd iteration and the k-means built on it.  References are NumPy only.

The rounding bound used throughout: d2 = |q|^2 + |t|^2 - 2 q.t evaluated in fp32 in ANY summation order differs
from its exact value by at most

    tau(q) = 2 (D + 3) 2^-24 (|q|^2 + max_t |t|^2)

(each of the three D-term sums carries at most D roundings of relative size 2^-24 on terms bounded by |q|^2, |t|^2
and |q||t| <= (|q|^2 + |t|^2) / 2, twice; three more roundings combine them).  It is derived, not measured."""
import functools

import numpy as np
import pytest
import torch

from han_amd import evaluate, ops

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def _t(a, dev):
    return torch.tensor(np.ascontiguousarray(a)).to(dev)


def _ints(rs, shape, r):
    return rs.randint(-r, r + 1, size=shape).astype(np.float32)


def _sorted_topk(d, k):
    """indices and values of the k smallest entries per row under (value, index)"""
    order = np.argsort(d, axis=1, kind="stable")[:, :k]
    return order, np.take_along_axis(d, order, axis=1)


def _d2_exact(q, t):
    q, t = q.astype(np.int64), t.astype(np.int64)
    return (q * q).sum(1)[:, None] + (t * t).sum(1)[None, :] - 2 * (q @ t.T)


def _d2_f64(q, t):
    q, t = q.astype(np.float64), t.astype(np.float64)
    return ((q[:, None, :] - t[None, :, :]) ** 2).sum(-1) if q.shape[0] * t.shape[0] * q.shape[1] < 5e7 else \
        np.stack([((t - row) ** 2).sum(1) for row in q])


def _tau(q, t):
    d = q.shape[1]
    qn = (q.astype(np.float64) ** 2).sum(1)
    return 2 * (d + 3) * U * (qn + (t.astype(np.float64) ** 2).sum(1).max())


# ------------------------------------------------------------------------------------------------ test 1: KNN, exact
# (Nq, Nt, D, k, value range, duplicated rows)
EXACT = [(257, 4099, 64, 5, 8, False), (257, 4099, 13, 16, 8, True), (37, 1000, 130, 1, 8, False),
         (37, 1000, 8, 5, 8, True), (37, 16, 13, 16, 8, False), (257, 200, 13, 5, 8, False),
         (257, 4099, 8, 5, 2, False), (37, 1000, 64, 16, 8, False)]


@pytest.mark.parametrize("nq,nt,d,k,r,dup", EXACT)
def test_knn_topk_is_exact_on_integer_rows(dev, nq, nt, d, k, r, dup):
    """Integer rows in [-8, 8]: d2 <= 130 * 256 < 2^24 and every partial sum is an integer, so any evaluation order
    is exact and idx / d2 must equal NumPy's int64 distances sorted by (d2, index), element for element."""
    rs = np.random.RandomState(nq + nt + d + k + r)
    q, t = _ints(rs, (nq, d), r), _ints(rs, (nt, d), r)
    if dup:
        t[nt // 2:nt // 2 + nt // 4] = t[:nt // 4]          # every such row ties with its copy for every query
    ref = _d2_exact(q, t)
    want_idx, want_d2 = _sorted_topk(ref, k)
    if r == 2 and nt > k:                                    # condition on the inputs: the tie rule decides most rows
        kth = np.sort(ref, axis=1)[:, k - 1:k + 1]
        assert (kth[:, 0] == kth[:, 1]).mean() > 0.5
    idx, d2 = ops.knn_topk(_t(q, dev), _t(t, dev), k)
    assert idx.dtype == torch.int32 and d2.dtype == torch.float32 and tuple(idx.shape) == (nq, k)
    np.testing.assert_array_equal(idx.cpu().numpy(), want_idx)
    np.testing.assert_array_equal(d2.cpu().numpy().astype(np.int64), want_d2)


def test_knn_topk_takes_strided_rows_and_no_queries(dev):
    rs = np.random.RandomState(3)
    big_q, big_t = _ints(rs, (40, 24), 8), _ints(rs, (300, 20), 8)
    q, t = big_q[:, 3:16], big_t[:, 5:18]                   # leading dimensions 24 and 20, width 13
    want_idx, _ = _sorted_topk(_d2_exact(q, t), 4)
    idx, _ = ops.knn_topk(_t(big_q, dev)[:, 3:16], _t(big_t, dev)[:, 5:18], 4)
    np.testing.assert_array_equal(idx.cpu().numpy(), want_idx)
    idx, d2 = ops.knn_topk(_t(q[:0], dev), _t(t, dev), 4)
    assert tuple(idx.shape) == (0, 4) and tuple(d2.shape) == (0, 4)
    for bad_k in (0, 17, 301):
        with pytest.raises(ValueError):
            ops.knn_topk(_t(q, dev), _t(t, dev), bad_k)


# ------------------------------------------------------------------------------------- tests 2, 3, 6: real-valued KNN
REAL = [(257, 4099, 64, 5), (257, 4099, 13, 5), (257, 4099, 64, 16), (37, 1000, 130, 1)]


@functools.lru_cache(maxsize=None)
def _real_case(nq, nt, d, k):
    rs = np.random.RandomState(1000 + d + k)
    q, t = rs.standard_normal((nq, d)).astype(np.float32), rs.standard_normal((nt, d)).astype(np.float32)
    labels = rs.randint(0, 4, nt).astype(np.int32)
    ref = _d2_f64(q, t)
    for a in (q, t, labels, ref):
        a.setflags(write=False)
    return q, t, labels, ref


@functools.lru_cache(maxsize=None)
def _real_result(nq, nt, d, k):
    q, t, _, _ = _real_case(nq, nt, d, k)
    dev = torch.device("cuda:0")
    idx, d2 = ops.knn_topk(_t(q, dev), _t(t, dev), k)
    return idx, d2


@pytest.mark.parametrize("nq,nt,d,k", REAL)
def test_knn_topk_real_valued_within_the_rounding_envelope(dev, nq, nt, d, k):
    q, t, _, ref = _real_case(nq, nt, d, k)
    tau = _tau(q, t)
    idx_t, d2_t = _real_result(nq, nt, d, k)
    idx, d2 = idx_t.cpu().numpy().astype(np.int64), d2_t.cpu().numpy().astype(np.float64)
    assert idx.min() >= 0 and idx.max() < nt
    true = np.take_along_axis(ref, idx, axis=1)
    kth = np.sort(ref, axis=1)[:, k - 1]
    assert (true <= (kth + tau)[:, None]).all()                       # every neighbour is a k nearest one up to tau
    assert (np.abs(d2 - true) <= tau[:, None]).all()                  # every distance is within tau
    assert all(len(set(row)) == k for row in idx)                     # distinct
    if k > 1:                                                         # ascending in the returned (d2, idx)
        dd, di = np.diff(d2, axis=1), np.diff(idx, axis=1)
        assert ((dd > 0) | ((dd == 0) & (di > 0))).all()


def _vote(lab):
    return np.array([np.bincount(row).argmax() for row in lab], dtype=np.int32)


@pytest.mark.parametrize("nq,nt,d,k", REAL)
def test_knn_vote_matches_the_float64_reference(dev, nq, nt, d, k):
    """Predictions equal the float64 reference's wherever the reference's neighbour SET is beyond doubt: the
    (k+1)-th distance exceeds the k-th by more than 2 tau.  At most 5 % of the queries may be left out."""
    q, t, labels, ref = _real_case(nq, nt, d, k)
    tau = _tau(q, t)
    order = np.argsort(ref, axis=1, kind="stable")
    srt = np.take_along_axis(ref, order[:, :k + 1], axis=1)
    sure = (srt[:, k] - srt[:, k - 1]) > 2 * tau
    assert (~sure).mean() <= 0.05
    want = _vote(labels[order[:, :k]])
    idx, _ = _real_result(nq, nt, d, k)
    pred = ops.knn_vote(idx, _t(labels, dev)).cpu().numpy()
    np.testing.assert_array_equal(pred[sure], want[sure])


def test_knn_vote_ties_go_to_the_smallest_class(dev):
    labels = np.array([2, 2, 1, 1, 0, 7, 7, 7, 3], dtype=np.int32)
    idx = np.array([[0, 1, 2, 3, 4], [4, 5, 0, 6, 1], [8, 4, 2, 0, 5], [5, 6, 7, 0, 1]], dtype=np.int32)
    pred = ops.knn_vote(_t(idx, dev), _t(labels, dev)).cpu().numpy()
    np.testing.assert_array_equal(pred, [1, 2, 0, 7])
    pred = ops.knn_vote(_t(idx[:, :1], dev), _t(labels, dev)).cpu().numpy()
    np.testing.assert_array_equal(pred, [2, 0, 3, 7])


@pytest.mark.parametrize("c", [1, 4, 64])
def test_contingency_is_exact(dev, c):
    rs = np.random.RandomState(c)
    n = 100003
    a, b = rs.randint(0, c, n).astype(np.int32), rs.randint(0, c, n).astype(np.int32)
    want = np.zeros((c, c), dtype=np.int64)
    np.add.at(want, (a, b), 1)
    got = ops.contingency(_t(a, dev), _t(b, dev), c, c)
    assert got.dtype == torch.int64 and not got.is_cuda
    np.testing.assert_array_equal(got.numpy(), want)
    bad = a.copy()
    bad[n // 2] = c
    with pytest.raises(ValueError):
        ops.contingency(_t(bad, dev), _t(b, dev), c, c)
    bad[n // 2] = -1
    with pytest.raises(ValueError):
        ops.contingency(_t(b, dev), _t(bad, dev), c, c)


def test_f1_and_nmi_ari_on_device_labels(dev):
    rs = np.random.RandomState(0)
    a = rs.randint(0, 5, 3001)
    b = np.where(rs.random_sample(3001) < 0.7, a, rs.randint(0, 4, 3001))
    t = np.zeros((5, 5), dtype=np.int64)
    np.add.at(t, (a, b), 1)
    assert evaluate.f1_scores(_t(a, dev), _t(b, dev)) == evaluate.f1_from_table(t)
    assert evaluate.f1_scores(a, b, n_classes=5) == evaluate.f1_from_table(t)
    assert evaluate.nmi_ari(_t(a, dev), b) == evaluate.nmi_ari_from_table(t)


# ----------------------------------------------------------------------------------------- test 4: kmeans_step, exact
@pytest.mark.parametrize("d", [13, 64])
@pytest.mark.parametrize("k", [1, 3, 4, 17, 64])
def test_kmeans_step_is_exact_on_integer_rows(dev, d, k):
    rs = np.random.RandomState(10 * d + k)
    n = 1003
    x, c = _ints(rs, (n, d), 8), _ints(rs, (k, d), 8)
    if k >= 3:
        c[1] = c[0]                     # a tie between two centres for every row: the smaller index wins
        c[k - 1] = 100.0                # far from every row: no rows, keeps its coordinates
    prev = rs.randint(0, k, n).astype(np.int32)
    ref = _d2_exact(x, c)
    want = ref.argmin(axis=1)
    want_d2 = ref.min(axis=1)
    step = ops.kmeans_step(_t(x, dev), _t(c, dev), _t(prev, dev))
    np.testing.assert_array_equal(step["labels"].cpu().numpy(), want)
    np.testing.assert_array_equal(step["d2"].cpu().numpy().astype(np.int64), want_d2)
    counts = np.bincount(want, minlength=k)
    np.testing.assert_array_equal(step["counts"].cpu().numpy(), counts)
    assert int(step["changed"]) == int((want != prev).sum())
    assert float(step["inertia"]) == float(want_d2.sum())
    new = step["centres"].cpu().numpy()
    for j in range(k):
        if counts[j]:
            mean = x[want == j].astype(np.float64).mean(axis=0)
            assert (np.abs(new[j].astype(np.float64) - mean) <= np.spacing(np.abs(mean).astype(np.float32))).all()
        else:
            np.testing.assert_array_equal(new[j], c[j])
    if k >= 3:
        assert counts[1] == 0 and counts[k - 1] == 0
    first = ops.kmeans_step(_t(x, dev), _t(c, dev), None, want_d2=False)
    assert first["d2"] is None and int(first["changed"]) == n
    np.testing.assert_array_equal(first["labels"].cpu().numpy(), want)


# ----------------------------------------------------------------------------------------------------- test 5: Lloyd
def _blobs(seed, n=1003, d=64, k=4):
    rs = np.random.RandomState(seed)
    centres = 0.5 * rs.standard_normal((k, d))
    y = rs.randint(0, k, n)
    return (centres[y] + rs.standard_normal((n, d))).astype(np.float32), y


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_lloyd_reaches_a_float64_fixed_point(dev, seed):
    x, _ = _blobs(seed)
    n, d = x.shape
    fit = evaluate.kmeans(_t(x, dev), 4, init=x[:4], tol=0)
    labels, centres = fit["labels"].cpu().numpy(), fit["centers"].cpu().numpy().astype(np.float64)
    np.testing.assert_array_equal(fit["init_centers"].cpu().numpy(), x[:4])
    assert fit["n_iter"] >= 3
    x64 = x.astype(np.float64)
    tau = 2 * (d + 3) * U * ((x64 ** 2).sum(1) + (centres ** 2).sum(1).max())
    # the bound of every iteration's centres: they are means of rows of x, so no longer than the longest row
    tau_any = 2 * (d + 3) * U * ((x64 ** 2).sum(1) + (x64 ** 2).sum(1).max())
    hist = fit["inertia_history"]
    assert len(hist) == fit["n_iter"] and hist[-1] == fit["inertia"]
    assert (np.diff(hist) <= tau_any.sum()).all()
    ref = _d2_f64(x, centres.astype(np.float32))
    srt = np.sort(ref, axis=1)
    sure = (srt[:, 1] - srt[:, 0]) > 2 * tau
    assert (~sure).mean() <= 0.01
    np.testing.assert_array_equal(labels[sure], ref.argmin(axis=1)[sure])
    for j in range(4):
        mean = x64[labels == j].mean(axis=0)
        assert (np.abs(centres[j] - mean) <= 2.0 ** -20 * np.abs(mean)).all()
    mine = ref[np.arange(n), labels].sum()
    assert abs(fit["inertia"] - mine) <= tau.sum()


def test_kmeans_seeding_is_reproducible(dev):
    x, _ = _blobs(7)
    xt = _t(x, dev)
    a, b = evaluate.kmeans(xt, 4, seed=5, n_init=2), evaluate.kmeans(xt, 4, seed=5, n_init=2)
    assert set(a) >= {"labels", "centers", "inertia", "n_iter", "init_centers"}
    assert a["inertia"] == b["inertia"] and a["n_iter"] == b["n_iter"]
    for key in ("labels", "centers", "init_centers"):
        assert torch.equal(a[key], b[key])
    init = a["init_centers"].cpu().numpy()
    assert init.shape == (4, 64)
    for row in init:
        assert (x == row).all(axis=1).any()
    assert len({r.tobytes() for r in init}) == 4


# ------------------------------------------------------------------------------------------------ test 6: determinism
def test_results_are_bitwise_reproducible(dev):
    q, t, _, _ = _real_case(*REAL[0])
    qt, tt = _t(q, dev), _t(t, dev)
    i1, d1 = ops.knn_topk(qt, tt, 5)
    i2, d2 = ops.knn_topk(qt, tt, 5)
    assert torch.equal(i1, i2) and torch.equal(d1.view(torch.int32), d2.view(torch.int32))
    c = tt[:17].contiguous()
    s1, s2 = ops.kmeans_step(tt, c), ops.kmeans_step(tt, c)
    for key in ("labels", "counts", "changed"):
        assert torch.equal(s1[key], s2[key])
    for key in ("d2", "centres"):
        assert torch.equal(s1[key].view(torch.int32), s2[key].view(torch.int32))
    assert torch.equal(s1["inertia"].view(torch.int64), s2["inertia"].view(torch.int64))


# ------------------------------------------------------------------------------------------------- test 7: end to end
def _planted(n=600, c=3, d=16):
    """integer-valued embeddings (every distance is exact in fp32 and in float64) of three overlapping classes"""
    rs = np.random.RandomState(42)
    y = rs.randint(0, c, n)
    centres = rs.randint(-40, 41, size=(c, d))
    return (centres[y] + rs.randint(-120, 121, size=(n, d))).astype(np.float64), y


def test_my_knn_and_my_kmeans_on_the_device(dev, capsys):
    x, y = _planted()
    knn = evaluate.my_KNN(x, np.eye(3)[y], time=2, seed=0, device=dev)
    assert set(knn) == {0.2, 0.4, 0.6, 0.8}
    assert all(isinstance(v, tuple) and len(v) == 2 and all(isinstance(s, float) and 0.0 <= s <= 1.0 for s in v)
               for v in knn.values())
    res = evaluate.my_Kmeans(_t(x.astype(np.float32), dev), y, k=3, time=2, seed=0, device=dev)
    assert isinstance(res, tuple) and len(res) == 2 and all(isinstance(s, float) for s in res)
    assert -1.0 <= res[1] <= 1.0 and 0.0 <= res[0] <= 1.0
    lines = capsys.readouterr().out.strip().split("\n")
    assert len(lines) == 5 and lines[0].startswith("KNN(2avg, split:0.2, k=5) f1_macro: ")
    assert lines[4].startswith("NMI (10 avg): ")


def test_my_knn_on_the_device_equals_the_sklearn_path(dev):
    pytest.importorskip("sklearn")
    x, y = _planted()
    want = evaluate.my_KNN(x, y, time=2, seed=0, verbose=False)
    got = evaluate.my_KNN(x, y, time=2, seed=0, verbose=False, device=dev)
    for ss in want:
        assert abs(got[ss][0] - want[ss][0]) <= 1e-12 and abs(got[ss][1] - want[ss][1]) <= 1e-12, (ss, got, want)
