"""The t-SNE kernels (han_tsne_calibrate / han_tsne_step in han_amd/csrc/evaluate.hip) and their Python layers against
NumPy float64 (tests/tsne_ref.py, itself held against scikit-learn by tests/test_tsne_host.py).

The calibration is checked through its outputs: dmin and zsum within bounds DERIVED from the fp32 pair bound, and the
perplexity the kernel's beta realises on float64 distances within 1e-4 (the forward tolerance of DESIGN section 6).  The
step is checked apart from it: the reference is fed the kernel's own (beta, dmin, zsum).  The update rule is bit-equal
to its float32 restatement.  Exact t-SNE is chaotic (two runs part after about 50 iterations at any precision), so
nothing compares trajectories beyond three steps, and the end-to-end test compares with the POPULATIONS of the fixture
tests/golden/tsne_ref.npz, never with numbers of the device's own.

Shapes: 37 x 8 is under one tile; 130 x 13 has a ragged third row tile and a width that is no multiple of 4; 257 x 70 a
tail tile of one row and a ragged second 64-column stage; 600 x 130 three stages and (asserted from the split rule)
several column splits; N_BIG x 2 has the first row-tile count at which the column range is NOT split (integer points, so
the norm form of d2 loses nothing to cancellation at this density), checked on 32 sampled rows.  "dup" has groups of
three bit-identical rows (dmin = 0, equal nearest neighbours), "x10" the 257-row case scaled by 10 (beta near 1 / 100).

A departure from the plan of this suite: the big case's Z_q is NOT a blocked float64 sum over its 10^9 pairs
(ref.zq_blocked takes 6 to 8 s there) but the exact sum ref.zq_lattice, which needs y on an integer lattice: the pairs
at every offset are counted by an autocorrelation of the occupancy histogram.  tests/test_tsne_host.py holds the two
sums against each other at 700 points.  The price is that the big case's y is integer-valued (about 1000 of its rows
share a point with another, w = 1 there); real-valued y is covered by every small case."""
import functools
import os

import numpy as np
import pytest
import torch

from han_amd import _lib, evaluate, ops
from tests import tsne_ref as ref

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tsne_ref.npz")


def splits(n):
    """column splits of an n-row call: knn_splits(N, N) of evaluate.hip (64-row tiles, about 512 workgroups, splits of
    a multiple of 256 rows, at most 64)"""
    row_tiles, units = -(-n // 64), -(-n // 256)
    ns = max(1, min(-(-512 // row_tiles), units, 64))
    return -(-n // (-(-units // ns) * 256))


N_BIG = 511 * 64 + 35      # 512 row tiles, the last of 35 rows
LATTICE = 1024             # the big case's y: integer points in [0, 1024)^2, whose Z_q is exact (ref.zq_lattice)

# name -> (rows, width, scale, duplicates)
CASES = {
    "37x8": (37, 8, 1.0, False),
    "130x13": (130, 13, 1.0, False),
    "257x70": (257, 70, 1.0, False),
    "600x130": (600, 130, 1.0, False),
    "dup": (130, 13, 1.0, True),
    "x10": (257, 70, 10.0, False),
}
PERPLEXITIES = (10.0, 30.0, 50.0)
CALIB = [(name, p) for name in CASES for p in PERPLEXITIES if p < CASES[name][0]]      # 50 >= 37 is no perplexity of 37 rows


def _t(a, dev):
    return torch.tensor(np.ascontiguousarray(a)).to(dev)


def _np(t):
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _case(name):
    """(x fp32, d2 float64, tau) of a small case, read-only"""
    n, dim, scale, dup = CASES[name]
    x = ref.blobs(n + dim, n, dim, spread=1.5)[0] * np.float32(scale)
    if dup:
        x[[40, 90]] = x[3]
        x[[41, 129]] = x[64]
    d2, tau = ref.d2_rows(x), ref.tau_rows(x)
    for a in (x, d2, tau):
        a.setflags(write=False)
    return x, d2, tau


@functools.lru_cache(maxsize=None)
def _calib(name, perplexity):
    return ops.tsne_calibrate(_t(_case(name)[0], torch.device("cuda:0")), perplexity)


def _start(name, kind):
    """(N, 2) fp32: "wide" is standard normal x 10, "init" scikit-learn's 1e-4 start"""
    n = CASES[name][0]
    z = np.random.RandomState(n).standard_normal((n, 2)).astype(np.float32)
    return z * np.float32(10.0 if kind == "wide" else 1e-4)


def _run_step(name, perplexity, y, update, gains, exaggeration, momentum, lr, want_grad=True, want_kl=True):
    """one ops.tsne_step on copies; everything it wrote as NumPy"""
    dev = torch.device("cuda:0")
    yt, ut, gt = _t(y, dev), _t(update, dev), _t(gains, dev)
    r = ops.tsne_step(_t(_case(name)[0], dev), _calib(name, perplexity), yt, ut, gt, exaggeration, momentum, lr,
                      want_grad=want_grad, want_kl=want_kl)
    return dict(y=_np(yt), update=_np(ut), gains=_np(gt), stats=_np(r["stats"]),
                grad=_np(r["grad"]) if want_grad else None)


def test_the_split_rule_reaches_both_paths():
    assert splits(600) >= 2 and splits(37) == 1
    assert splits(N_BIG) == 1 and splits(N_BIG - 64) >= 2      # the first row count of its tile remainder that is not split
    lib = _lib.load()
    for n in (600, N_BIG):                                      # the slabs the library sizes are those of this rule
        assert lib.han_tsne_workspace(n, 64) >= splits(n) * 7 * 8 * n
        assert lib.han_tsne_workspace(n, 64) < (splits(n) + 1) * 7 * 8 * n + (1 << 16)


@pytest.mark.parametrize("name,perplexity", CALIB)
def test_calibration_within_the_derived_bounds(dev, name, perplexity):
    x, d2, tau = _case(name)
    n = x.shape[0]
    c = _calib(name, perplexity)
    beta, dmin, zsum = (_np(c[key]).astype(np.float64) for key in ("beta", "dmin", "zsum"))
    assert c["beta"].dtype == torch.float32 and c["state"].dtype == torch.float64 and c["state"].shape == (3, n)
    print("passes %d, open rows %d" % (int(c["passes"]), int(c["open_rows"].cpu()[0])))
    assert int(c["open_rows"].cpu()[0]) == 0 and int(c["passes"]) <= 100
    assert (_np(c["state"])[0] == -beta).all()                  # every row closed, at the beta it reports
    want = ref.calib_bounds(d2, tau, np.arange(n), beta, dmin)
    print("max |dmin - ref| / bound %.3g, max |zsum - ref| / bound %.3g" % (
        (np.abs(dmin - want["dmin"]) / want["e_dmin"]).max(), (np.abs(zsum - want["zsum"]) / want["e_zsum"]).max()))
    assert (np.abs(dmin - want["dmin"]) <= want["e_dmin"]).all()
    assert (np.abs(zsum - want["zsum"]) <= want["e_zsum"]).all()
    assert (zsum >= 1.0).all()                                  # the nearest neighbour's term is exactly 1
    if CASES[name][3]:
        assert (dmin[[3, 40, 90, 64, 41, 129]] <= want["e_dmin"][[3, 40, 90, 64, 41, 129]]).all()
    err = np.abs(want["perplexity"] / perplexity - 1.0).max()
    print("max |realised perplexity / %g - 1| = %.3g" % (perplexity, err))
    assert err <= 1e-4


@pytest.mark.parametrize("exaggeration", [12.0, 1.0])
@pytest.mark.parametrize("kind", ["wide", "init"])
@pytest.mark.parametrize("name", list(CASES))
def test_step_against_float64_fed_the_kernels_calibration(dev, name, kind, exaggeration):
    x, d2, _ = _case(name)
    n = x.shape[0]
    c = _calib(name, 10.0)
    y0 = _start(name, kind)
    zeros, ones = np.zeros((n, 2), np.float32), np.ones((n, 2), np.float32)
    lr = max(n / 12.0 / 4.0, 50.0)
    got = _run_step(name, 10.0, y0, zeros, ones, exaggeration, 0.5, lr)
    p = ref.joint_rows(d2, np.arange(n), *(_np(c[key]) for key in ("beta", "dmin", "zsum")))
    grad, _, kl_rows, zq = ref.step_rows(p, y0, None, exaggeration)
    kl = kl_rows.sum()
    g_err = np.abs(got["grad"] - grad).max() / np.abs(grad).max()
    print("grad: relative max-norm error %.3g; Z_q %.3g; KL %.3g" % (
        g_err, abs(got["stats"][0] / zq - 1), abs(got["stats"][2] - kl)))
    assert got["grad"].dtype == np.float32 and g_err <= 2e-3
    assert abs(got["stats"][0] - zq) <= 1e-4 * zq
    assert abs(got["stats"][2] - kl) <= 1e-4 * max(1.0, abs(kl))            # relative / absolute
    gg = (got["gains"] * got["grad"]).astype(np.float64)                      # the fp32 product, as the kernel forms it
    assert abs(got["stats"][1] - (gg ** 2).sum()) <= 1e-9 * min(1.0, (gg ** 2).sum())
    # the update rule, bit for bit, from the kernel's own gradient
    want = ref.update_rule(y0, zeros, ones, got["grad"], 0.5, lr, dtype=np.float32)
    for key, w in zip(("y", "update", "gains"), want):
        assert np.array_equal(got[key], w), key
    # neither want_kl = 0 nor grad = NULL changes another output bit; stats[2] is left as it was
    plain = _run_step(name, 10.0, y0, zeros, ones, exaggeration, 0.5, lr, want_grad=True, want_kl=False)
    bare = _run_step(name, 10.0, y0, zeros, ones, exaggeration, 0.5, lr, want_grad=False, want_kl=True)
    assert np.isnan(plain["stats"][2]) and np.array_equal(plain["grad"], got["grad"])
    assert bare["stats"][2] == got["stats"][2]
    for other in (plain, bare):
        assert np.array_equal(other["stats"][:2], got["stats"][:2])
        for key in ("y", "update", "gains"):
            assert np.array_equal(other[key], got[key]), key


@pytest.mark.parametrize("name", ["130x13", "600x130"])
def test_second_step_with_momentum_and_a_clamped_gain_is_bit_equal(dev, name):
    n = CASES[name][0]
    rs = np.random.RandomState(n + 1)
    y0 = _start(name, "wide")
    update = rs.standard_normal((n, 2)).astype(np.float32)
    gains = np.where(rs.rand(n, 2) < 0.3, 0.0121, 1.0 + rs.rand(n, 2)).astype(np.float32)      # 0.0121 * 0.8 < min_gain
    first = _run_step(name, 10.0, y0, update, gains, 1.0, 0.8, 50.0)
    want = ref.update_rule(y0, update, gains, first["grad"], 0.8, 50.0, dtype=np.float32)
    assert (want[2] == np.float32(0.01)).any() and (want[2] > gains).any() and (want[2] < gains).any()
    for key, w in zip(("y", "update", "gains"), want):
        assert np.array_equal(first[key], w), key
    second = _run_step(name, 10.0, first["y"], first["update"], first["gains"], 1.0, 0.8, 50.0)
    want2 = ref.update_rule(first["y"], first["update"], first["gains"], second["grad"], 0.8, 50.0, dtype=np.float32)
    for key, w in zip(("y", "update", "gains"), want2):
        assert np.array_equal(second[key], w), key


@pytest.mark.parametrize("name", list(CASES))
def test_three_steps_against_float64(dev, name):
    x, d2, _ = _case(name)
    n = x.shape[0]
    c = _calib(name, 10.0)
    lr = max(n / 12.0 / 4.0, 50.0)
    y0 = _start(name, "init")
    state = dict(y=y0, update=np.zeros((n, 2), np.float32), gains=np.ones((n, 2), np.float32))
    for _ in range(3):
        state = _run_step(name, 10.0, state["y"], state["update"], state["gains"], 12.0, 0.5, lr, False, False)
    p = ref.joint_rows(d2, np.arange(n), *(_np(c[key]) for key in ("beta", "dmin", "zsum")))
    want, _ = ref.descend(p, y0, 3, 12.0, 0.5, lr)
    err = np.abs(state["y"] - want).max() / np.abs(want).max()
    print("three steps: relative max-norm difference %.3g" % err)
    assert err <= 1e-4


@functools.lru_cache(maxsize=None)
def _big():
    rs = np.random.RandomState(N_BIG)
    x = rs.randint(0, 1024, (N_BIG, 2)).astype(np.float32)      # integers: every fp32 d2 is exact, as the norms stay below 2^24
    y = rs.randint(0, LATTICE, (N_BIG, 2)).astype(np.float32)
    rows = np.sort(np.concatenate([[0, N_BIG - 1], rs.choice(np.arange(1, N_BIG - 1), 30, replace=False)]))
    for a in (x, y, rows):
        a.setflags(write=False)
    return x, y, rows, ops.tsne_calibrate(_t(x, torch.device("cuda:0")), 30.0)


def test_unsplit_shape_on_sampled_rows(dev):
    x, y, rows, c = _big()
    beta, dmin, zsum = (_np(c[key]).astype(np.float64) for key in ("beta", "dmin", "zsum"))
    print("passes %d" % int(c["passes"]))
    assert int(c["open_rows"].cpu()[0]) == 0 and int(c["passes"]) <= 100
    d2 = ref.d2_rows(x, rows)
    want = ref.calib_bounds(d2, ref.tau_rows(x, rows), rows, beta, dmin)
    assert (np.abs(dmin[rows] - want["dmin"]) <= want["e_dmin"]).all()
    assert (np.abs(zsum[rows] - want["zsum"]) <= want["e_zsum"]).all()
    err = np.abs(want["perplexity"] / 30.0 - 1.0).max()
    print("max |realised perplexity / 30 - 1| = %.3g" % err)
    assert err <= 1e-4
    yt = _t(y, dev)
    ut, gt = torch.zeros_like(yt), torch.ones_like(yt)
    r = ops.tsne_step(_t(x, dev), c, yt, ut, gt, 1.0, 0.8, 200.0, want_grad=True)
    zq = ref.zq_lattice(y, LATTICE)
    grad = ref.step_rows(ref.joint_rows(d2, rows, beta, dmin, zsum), y, rows, 1.0, zq)[0]
    got = _np(r["grad"])
    g_err = np.abs(got[rows] - grad).max() / np.abs(grad).max()
    print("grad (32 rows): relative max-norm error %.3g; Z_q %.3g" % (g_err, abs(float(r["stats"][0]) / zq - 1)))
    assert g_err <= 2e-3 and abs(float(r["stats"][0]) - zq) <= 1e-4 * zq
    upd = ref.update_rule(y, np.zeros_like(y), np.ones_like(y), got, 0.8, 200.0, dtype=np.float32)
    assert np.array_equal(_np(yt), upd[0]) and np.array_equal(_np(gt), upd[2])


def test_two_runs_are_bitwise_equal(dev):
    for name in ("600x130", "37x8"):
        x = _t(_case(name)[0], dev)
        n = x.shape[0]
        first, again = _calib(name, 10.0), ops.tsne_calibrate(x, 10.0)
        for key in ("beta", "dmin", "zsum", "state", "open_rows"):
            assert torch.equal(first[key], again[key]), (name, key)
        runs = []
        for _ in range(2):
            y = _t(_start(name, "init"), dev)
            u, g = torch.zeros_like(y), torch.ones_like(y)
            for i in range(20):
                r = ops.tsne_step(x, first, y, u, g, 12.0, 0.5, 50.0, want_grad=True, want_kl=i % 2 == 0)
            runs.append((y, u, g, r["grad"], r["stats"][:2]))
        for a, b in zip(*runs):
            assert torch.equal(a, b), name
    x, y0, _, c = _big()
    again = ops.tsne_calibrate(_t(x, dev), 30.0)
    for key in ("beta", "dmin", "zsum", "state"):
        assert torch.equal(c[key], again[key]), key


def test_strided_rows(dev):
    x = _case("257x70")[0]
    big = np.full((257, 80), 99.0, dtype=np.float32)
    big[:, 5:75] = x
    view = _t(big, dev)[:, 5:75]
    assert view.stride(0) == 80
    c, s = _calib("257x70", 10.0), ops.tsne_calibrate(view, 10.0)
    for key in ("beta", "dmin", "zsum"):
        assert torch.equal(c[key], s[key]), key
    outs = []
    for xt in (_t(x, dev), view):
        y = _t(_start("257x70", "wide"), dev)
        r = ops.tsne_step(xt, c, y, torch.zeros_like(y), torch.ones_like(y), 1.0, 0.8, 50.0, want_grad=True, want_kl=True)
        outs.append((y, r["grad"], r["stats"]))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


@pytest.fixture(scope="module")
def fix():
    f = np.load(GOLDEN)
    p = ref.joint(ref.d2_rows(f["x"]), 30.0)[0]
    p.setflags(write=False)
    return f, p


@pytest.mark.parametrize("s", range(8))
def test_end_to_end_within_the_fixture_populations(dev, fix, s):
    f, p = fix
    kls = np.concatenate([f["kl_ref"], f["kl_sk"]])
    trusts = np.concatenate([f["trust_ref"], f["trust_sk"]])
    y, info = evaluate.tsne(f["x"], perplexity=30.0, init=f["inits"][s], device=dev, return_info=True)
    assert y.is_cuda and y.dtype == torch.float32 and tuple(y.shape) == (300, 2)
    kl, trust = ref.kl_of(p, _np(y)), ref.trustworthiness(f["x"], _np(y))
    print("seed %d: KL %.4f (fixture %.4f .. %.4f), trustworthiness %.4f (fixture %.4f .. %.4f), n_iter %d, reported KL "
          "%.6f, calibration passes %d" % (s, kl, kls.min(), kls.max(), trust, trusts.min(), trusts.max(), info["n_iter"],
                                           info["kl_divergence"], info["calibration_passes"]))
    assert kl <= kls.max() + (kls.max() - kls.min())
    assert trust >= trusts.min() - (trusts.max() - trusts.min())
    assert info["open_rows"] == 0 and 250 < info["n_iter"] <= 1000
    assert np.isfinite(info["kl_divergence"]) and abs(info["kl_divergence"] - kl) <= 1e-4


def test_python_layer(dev):
    f = np.load(GOLDEN)
    x = _t(f["x"], dev)
    y = evaluate._tsne_init(x, "pca", None, dev)
    yc = _np(y).astype(np.float64)
    assert y.is_cuda and y.dtype == torch.float32 and tuple(y.shape) == (300, 2)
    assert abs(yc[:, 0].std() / 1e-4 - 1) <= 1e-5 and yc[:, 0].std() >= yc[:, 1].std()
    assert abs((yc[:, 0] * yc[:, 1]).sum()) <= 1e-5 * np.sqrt((yc[:, 0] ** 2).sum() * (yc[:, 1] ** 2).sum())
    assert abs(yc.mean(0)).max() <= 1e-9
    r = np.float32(1e-4) * np.random.RandomState(6).standard_normal(size=(300, 2)).astype(np.float32)
    assert np.array_equal(_np(evaluate._tsne_init(x, "random", 6, dev)), r)
    short = evaluate.tsne(x, max_iter=60, device=dev)                   # pca start, a GPU tensor in
    assert short.is_cuda and short.device == x.device and bool(torch.isfinite(short).all())
    with pytest.raises(ValueError, match="perplexity"):
        evaluate.tsne(x[:30], perplexity=30.0, device=dev)
    with pytest.raises(ValueError, match="at most 512"):
        evaluate.tsne(torch.zeros((40, 513), device=dev), perplexity=5.0, device=dev)
    with pytest.raises(ValueError, match="CPU tensor"):
        evaluate.tsne(x.cpu(), device=dev)
    with pytest.raises(ValueError, match="learning_rate"):
        evaluate.tsne(x, learning_rate="atuo", device=dev)
    with pytest.raises(ValueError):
        evaluate.tsne(x, init=np.zeros((299, 2), np.float32), device=dev)
    with pytest.raises(ValueError):
        evaluate.tsne(x[:1], perplexity=1.0, device=dev)                # one row: no perplexity below n
    two, info = evaluate.tsne(x[:2], perplexity=1.0, init="random", seed=0, max_iter=20, device=dev, return_info=True)
    assert tuple(two.shape) == (2, 2) and bool(torch.isfinite(two).all()) and info["open_rows"] == 0
    one = ops.tsne_calibrate(x[:1], 1.0)
    assert int(one["passes"]) == 0 and one["beta"].shape == (1,)
    y1 = torch.ones((1, 2), device=dev)
    r1 = ops.tsne_step(x[:1], one, y1, torch.zeros_like(y1), torch.ones_like(y1), 1.0, 0.5, 50.0)
    assert float(r1["stats"][0]) == 0.0 and bool((y1 == 1).all())       # N = 1: nothing is launched


def test_errors(dev):
    x = _t(_case("37x8")[0], dev)
    c = _calib("37x8", 10.0)
    y = torch.zeros((37, 2), device=dev)
    with pytest.raises(ValueError):
        ops.tsne_calibrate(x, 37.0)
    with pytest.raises(ValueError):
        ops.tsne_calibrate(x.cpu(), 10.0)
    with pytest.raises(ValueError):
        ops.tsne_calibrate(x, 10.0, max_passes=0)                       # nothing evaluated: no beta to return
    with pytest.raises(ValueError):
        ops.tsne_step(x, c, y[:36], y, y, 1.0, 0.5, 50.0)
    with pytest.raises(ValueError):
        ops.tsne_step(x, c, y, y, y, 0.0, 0.5, 50.0)
    lib = _lib.load()
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
    state = torch.zeros((3, 37), dtype=torch.float64, device=dev)
    stats = torch.full((3,), 7.0, dtype=torch.float64, device=dev)
    opened = torch.zeros(1, dtype=torch.int64, device=dev)
    b, m, z = (torch.zeros(37, device=dev) for _ in range(3))
    u, g = torch.zeros_like(y), torch.ones_like(y)
    cal = (b.data_ptr(), m.data_ptr(), z.data_ptr(), state.data_ptr(), opened.data_ptr())
    assert lib.han_tsne_calibrate(x.data_ptr(), 8, 37, 8, 10.0, 1e-5, 1, 1, *cal, ws.data_ptr(), 16, None) == -3      # HAN_E_WORKSPACE
    for bad in (37.0, 0.5, float("nan"), float("inf")):                 # perplexity: finite, >= 1, < N; all else is valid here
        assert lib.han_tsne_calibrate(x.data_ptr(), 8, 37, 8, bad, 1e-5, 1, 1, *cal, ws.data_ptr(), ws.numel(), None) == -1
    assert lib.han_tsne_calibrate(x.data_ptr(), 8, 37, 8, 10.0, -1.0, 1, 1, *cal, ws.data_ptr(), ws.numel(), None) == -1
    assert lib.han_tsne_calibrate(x.data_ptr(), 8, 37, 8, 10.0, 1e-5, 1, 1, *cal[:4], None, ws.data_ptr(), ws.numel(), None) == -1
    step = (c["beta"].data_ptr(), c["dmin"].data_ptr(), c["zsum"].data_ptr(), y.data_ptr(), u.data_ptr(), g.data_ptr(), None)
    tail = (37, 8, 1.0, 0.5, 50.0, 0.01, 0)
    assert lib.han_tsne_step(x.data_ptr(), 8, *step, stats.data_ptr(), *tail, ws.data_ptr(), 16, None) == -3
    assert lib.han_tsne_step(x.data_ptr(), 8, *step, None, *tail, ws.data_ptr(), ws.numel(), None) == -1
    assert lib.han_tsne_step(x.data_ptr(), 8, *step, stats.data_ptr(), 1, 8, 1.0, 0.5, 50.0, 0.01, 1, ws.data_ptr(), ws.numel(),
                             None) == 0                                 # N = 1
    torch.cuda.synchronize()
    assert (_np(stats) == 7.0).all() and (_np(y) == 0).all()            # nothing above wrote anything
    assert lib.han_tsne_step(x.data_ptr(), 8, *step, stats.data_ptr(), *tail, ws.data_ptr(), ws.numel(), None) == 0
    torch.cuda.synchronize()
    assert float(stats[2]) == 7.0 and float(stats[0]) == 36.0 * 37.0    # y = 0: every w is 1; want_kl = 0 leaves stats[2]
