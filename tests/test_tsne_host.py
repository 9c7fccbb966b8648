"""The host side of the t-SNE evaluation: the float64 reference of the GPU tests (tests/tsne_ref.py) against
scikit-learn's own functions, the ABI 13 entry points' argument checks, and evaluate.tsne(device=None).
tests/golden/tsne_ref.npz is written by tests/golden/gen_tsne_fixture.py.  No GPU."""
import os

import numpy as np
import pytest

from han_amd import _lib, evaluate
from tests import tsne_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tsne_ref.npz")
PERPLEXITY = 30.0


@pytest.fixture(scope="module")
def fix():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def joint(fix):
    d2 = ref.d2_rows(fix["x"])
    p, beta, passes = ref.joint(d2, PERPLEXITY)
    for a in (d2, p, beta):
        a.setflags(write=False)
    return d2, p, beta, passes


def test_fixture_holds_arrays_only(fix):
    assert sorted(fix.files) == ["inits", "kl_ref", "kl_sk", "labels", "seeds", "trust_ref", "trust_sk", "x"]
    assert fix["x"].shape == (300, 16) and fix["x"].dtype == np.float32
    assert fix["inits"].shape == (8, 300, 2) and fix["inits"].dtype == np.float32
    assert all(fix[key].dtype.kind in "fiu" for key in fix.files)
    assert all(fix[key].shape == (8,) for key in ("seeds", "kl_ref", "kl_sk", "trust_ref", "trust_sk"))
    assert os.path.getsize(GOLDEN) < 64 * 1024
    for s, y0 in zip(fix["seeds"], fix["inits"]):                       # scikit-learn's init="random" numbers
        want = np.float32(1e-4) * np.random.RandomState(int(s)).standard_normal(size=(300, 2)).astype(np.float32)
        assert np.array_equal(y0, want)


def test_bisection_reaches_the_perplexity(joint):
    d2, p, beta, passes = joint
    realised = np.exp(ref.entropy(d2, np.arange(300), beta)[0])
    print("passes %d, max |perplexity / %g - 1| = %.3g" % (passes, PERPLEXITY, np.abs(realised / PERPLEXITY - 1).max()))
    assert passes <= 100
    assert np.abs(realised / PERPLEXITY - 1).max() <= 1e-5
    assert abs(p.sum() - 1.0) <= 1e-12 and np.array_equal(p, p.T) and (np.diag(p) == 0).all()


def test_joint_probabilities_are_scikit_learns(fix, joint):
    """_joint_probabilities bisects on float32 distances with tol 1e-5 on the entropy; both P sum to 1, and a
    conditional row moves by at most about tol times its log range when the entropy moves by tol"""
    pytest.importorskip("sklearn")
    from scipy.spatial.distance import squareform
    from sklearn.manifold._t_sne import _joint_probabilities
    from sklearn.metrics import pairwise_distances
    d2, p, _, _ = joint
    dist = pairwise_distances(fix["x"], metric="euclidean", squared=True)
    p_sk = squareform(_joint_probabilities(dist, PERPLEXITY, 0))
    assert np.abs(p - p_sk).max() <= 1e-3 * p_sk.max()
    assert np.abs(p - p_sk).sum() <= 1e-3


@pytest.mark.parametrize("spread,exaggeration", [(10.0, 12.0), (1e-4, 1.0)])
def test_gradient_and_kl_are_kl_divergence(joint, spread, exaggeration):
    pytest.importorskip("sklearn")
    from scipy.spatial.distance import squareform
    from sklearn.manifold._t_sne import _kl_divergence
    _, p, _, _ = joint
    y = spread * np.random.RandomState(4).standard_normal((300, 2))
    kl_sk, grad_sk = _kl_divergence(y.ravel().copy(), squareform(exaggeration * p, checks=False), 1, 300, 2)
    grad, _, kl_rows, _ = ref.step_rows(p, y, None, exaggeration)
    assert abs(kl_rows.sum() - kl_sk) <= 1e-12 * abs(kl_sk)
    assert np.abs(grad.ravel() - grad_sk).max() <= 1e-12 * np.abs(grad_sk).max()


def test_ten_iterations_are_gradient_descent(fix, joint):
    pytest.importorskip("sklearn")
    from scipy.spatial.distance import squareform
    from sklearn.manifold._t_sne import _gradient_descent, _kl_divergence
    _, p, _, _ = joint
    y0 = fix["inits"][0].astype(np.float64)
    lr = max(300 / 12.0 / 4.0, 50.0)
    y_sk, _, it = _gradient_descent(_kl_divergence, y0.ravel().copy(), it=0, max_iter=10, n_iter_check=50, momentum=0.5,
                                    learning_rate=lr, min_gain=0.01, args=[squareform(12.0 * p, checks=False), 1, 300, 2])
    y, _ = ref.descend(p, y0, 10, 12.0, 0.5, lr)
    err = np.abs(y.ravel() - y_sk).max() / np.abs(y_sk).max()
    print("10 iterations: relative max-norm difference %.3g" % err)
    assert it == 9 and err <= 1e-9


def test_float32_update_rule_is_the_float64_one_rounded():
    rs = np.random.RandomState(9)
    y, upd, grad = (rs.standard_normal((50, 2)).astype(np.float32) for _ in range(3))
    gains = np.where(rs.rand(50, 2) < 0.3, 0.0121, 1.0 + rs.rand(50, 2)).astype(np.float32)      # 0.0121 * 0.8 < min_gain
    a = ref.update_rule(y, upd, gains, grad, 0.8, 50.0, dtype=np.float32)
    b = ref.update_rule(y, upd, gains, grad, 0.8, 50.0)
    assert all(v.dtype == np.float32 for v in a)
    assert (a[2] == np.float32(0.01)).any() and (a[2] > 1).any()
    for got, want in zip(a, b):
        assert np.abs(got - want).max() <= 4 * 2.0 ** -24 * np.abs(want).max() + 1e-9


def test_trustworthiness_and_the_fixture_populations(fix, joint):
    """the NumPy trustworthiness is scikit-learn's; the fixture's two KL populations are narrow and overlap, whichever
    implementation produced them"""
    pytest.importorskip("sklearn")
    from sklearn.manifold import trustworthiness
    _, p, _, _ = joint
    y = ref.tsne(p, fix["inits"][1], max_iter=60)
    assert abs(ref.trustworthiness(fix["x"], y) - trustworthiness(fix["x"], y, n_neighbors=5)) <= 1e-12
    kl = np.concatenate([fix["kl_ref"], fix["kl_sk"]])
    print("fixture KL %.4f .. %.4f, trustworthiness %.4f .. %.4f" % (
        kl.min(), kl.max(), min(fix["trust_ref"].min(), fix["trust_sk"].min()),
        max(fix["trust_ref"].max(), fix["trust_sk"].max())))
    assert np.isfinite(kl).all() and kl.max() - kl.min() < 0.1 * kl.min()
    assert abs(np.median(fix["kl_ref"]) - np.median(fix["kl_sk"])) <= kl.max() - kl.min()


def test_lattice_zq_is_the_blocked_sum():
    y = np.random.RandomState(2).randint(0, 64, (700, 2)).astype(np.float32)
    assert abs(ref.zq_lattice(y, 64) / ref.zq_blocked(y, block=256) - 1) <= 1e-13
    assert abs(ref.zq_blocked(y) / ref.step_rows(np.zeros((700, 700)), y)[3] - 1) <= 1e-13


def test_abi_13_declares_the_tsne_entry_points():
    assert _lib.ABI_VERSION >= 13
    assert {"han_tsne_workspace", "han_tsne_calibrate", "han_tsne_step"} <= set(_lib.SIGNATURES)
    lib = _lib.load()
    assert lib.han_tsne_workspace(4099, 64) >= 4099 * (4 + 7 * 8)      # norms, one slab of seven double sums
    assert lib.han_tsne_workspace(4099, 513) == 0 and lib.han_tsne_workspace(0, 64) == 0
    assert lib.han_tsne_workspace(2 ** 31, 64) == 0

    def calibrate(ldx, n, d, perplexity, tol=1e-5):
        return lib.han_tsne_calibrate(None, ldx, n, d, perplexity, tol, 1, 1, None, None, None, None, None, None, 0, None)

    def step(ldx, n, d, exaggeration=1.0):
        return lib.han_tsne_step(None, ldx, None, None, None, None, None, None, None, None, n, d, exaggeration, 0.5, 50.0,
                                 0.01, 0, None, 0, None)
    # argument checks that return before anything touches the device
    assert calibrate(8, 10, 8, 5.0) == -1 and step(8, 10, 8) == -1               # NULL pointers
    assert calibrate(4, 10, 8, 5.0) == -1 and step(4, 10, 8) == -1               # ldx < D
    assert calibrate(8, 10, 0, 5.0) == -1 and step(8, -1, 8) == -1
    for bad in (10.0, 0.5, float("nan"), float("inf")):                         # perplexity: finite, >= 1, < N (with
        assert calibrate(8, 10, 8, bad) == -1                                   # real pointers: tests/test_tsne_gpu.py)
    assert calibrate(513, 10, 513, 5.0) == -2 and step(513, 10, 513) == -2       # HAN_E_UNSUPPORTED
    assert calibrate(8, 2 ** 31, 8, 5.0) == -2 and step(8, 2 ** 31, 8) == -2
    assert calibrate(8, 1, 8, 5.0) == 0 and step(8, 1, 8) == 0                   # N <= 1: nothing to do
    assert calibrate(8, 0, 8, 5.0) == 0 and step(8, 0, 8) == 0


def test_host_tsne_is_scikit_learns(fix):
    pytest.importorskip("sklearn")
    from sklearn.manifold import TSNE
    x, y0 = fix["x"][:100], fix["inits"][3][:100]
    got, info = evaluate.tsne(x, perplexity=20.0, max_iter=300, init=y0, return_info=True)
    est = TSNE(n_components=2, method="exact", perplexity=20.0, max_iter=300, init=y0)
    want = est.fit_transform(x)
    assert isinstance(got, np.ndarray) and got.shape == (100, 2) and np.array_equal(got, want)
    assert info["kl_divergence"] == float(est.kl_divergence_) and info["n_iter"] == est.n_iter_
    seeded = evaluate.tsne(x, perplexity=20.0, max_iter=300, init="random", seed=3)
    assert np.array_equal(seeded, TSNE(n_components=2, method="exact", perplexity=20.0, max_iter=300, init="random",
                                       random_state=3).fit_transform(x))
    assert np.array_equal(seeded, got)                                  # seed 3: the fixture's inits[3]
    with pytest.raises(ValueError):
        evaluate.tsne(x, perplexity=100.0)
