"""Host side of the GPU evaluation path (han_amd/evaluate.py): the scores formed from a contingency table agree with
scikit-learn, the scikit-learn path of my_KNN / my_Kmeans is what it was, and argument errors are raised before any
library call (there is no GPU here)."""
import os
import warnings

import numpy as np
import pytest

from han_amd import evaluate


def _table(a, b, c):
    t = np.zeros((c, c), dtype=np.int64)
    np.add.at(t, (a, b), 1)
    return t


def _cases():
    rs = np.random.RandomState(5)
    out = []
    for c in (2, 3, 7):
        a, b = rs.randint(0, c, 400), rs.randint(0, c, 400)
        out.append((f"random C={c}", a, b, c))
        b2 = b.copy()
        b2[b2 == c - 1] = 0
        out.append((f"class missing from the predictions C={c}", a, b2, c))
        a2 = a.copy()
        a2[a2 == c - 1] = 0
        out.append((f"class missing from the truth C={c}", a2, b, c))
        b3 = np.where(rs.random_sample(400) < 0.8, a, b)            # mostly right: scores away from chance
        out.append((f"correlated C={c}", a, b3, c))
    z = np.zeros(50, dtype=np.int64)
    out.append(("both a single cluster", z, z, 3))
    out.append(("truth a single cluster", z, rs.randint(0, 3, 50), 3))
    out.append(("predictions a single cluster", rs.randint(0, 3, 50), z + 1, 3))
    return out


@pytest.mark.parametrize("name,a,b,c", _cases(), ids=[c[0] for c in _cases()])
def test_scores_from_a_table_match_sklearn(name, a, b, c):
    from sklearn.metrics import adjusted_rand_score, f1_score, normalized_mutual_info_score
    t = _table(a, b, c)
    macro, micro = evaluate.f1_from_table(t)
    nmi, ari = evaluate.nmi_ari_from_table(t)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                 # sklearn warns about a class without predictions
        ref = (f1_score(a, b, average="macro"), f1_score(a, b, average="micro"),
               normalized_mutual_info_score(a, b), adjusted_rand_score(a, b))
    for got, want in zip((macro, micro, nmi, ari), ref):
        assert isinstance(got, float) and abs(got - want) <= 1e-12, (name, got, want)


def test_single_cluster_nmi_is_one():
    assert evaluate.nmi_ari_from_table(np.array([[17]]))[0] == 1.0
    assert evaluate.nmi_ari_from_table(np.array([[0, 0], [0, 9]])) == (1.0, 1.0)


def test_sklearn_path_is_unchanged_by_the_device_argument(capsys):
    """device=None (the default) is the scikit-learn path of the reference: the values of tests/golden/jhyexp_ref.npz,
    which the reference's own functions produced, and the same printed lines."""
    import sklearn
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "jhyexp_ref.npz"))
    if str(z["sklearn_version"]) != sklearn.__version__:
        pytest.skip("fixture was generated with another scikit-learn")
    x, y, seed, time = z["x"], z["y"], int(z["seed"]), int(z["time"])
    knn = evaluate.my_KNN(x, np.eye(int(z["k_means"]))[y], k=int(z["k_knn"]), time=time, seed=seed, device=None)
    for split, macro, micro in z["knn"]:
        got = knn[float(split)]
        assert abs(got[0] - macro) < 6e-5 and abs(got[1] - micro) < 6e-5, (split, got, macro, micro)
    nmi, ari = evaluate.my_Kmeans(x, y, k=int(z["k_means"]), time=time, seed=seed, device=None)
    assert abs(nmi - z["kmeans"][0]) < 1e-12 and abs(ari - z["kmeans"][1]) < 1e-12
    lines = capsys.readouterr().out.strip().split("\n")
    assert len(lines) == 5
    assert lines[0].startswith("KNN(3avg, split:0.2, k=5) f1_macro: ") and lines[4].startswith("NMI (10 avg): ")
    again = evaluate.my_KNN(x, np.eye(int(z["k_means"]))[y], k=int(z["k_knn"]), time=time, seed=seed, verbose=False)
    assert again == knn


@pytest.fixture
def no_library(monkeypatch):
    """Any call into the library or onto a device fails the test."""
    from han_amd import _lib

    def boom(*a, **k):
        raise AssertionError("the library was reached before the arguments were checked")
    monkeypatch.setattr(_lib, "load", boom)
    monkeypatch.setattr(evaluate, "_embed", boom)
    monkeypatch.setattr(evaluate, "_labels", boom)


@pytest.mark.parametrize("k", [0, -1, 17, 11, 2.5])
def test_knn_argument_errors(no_library, k):
    x_train, y_train, x_test = np.zeros((10, 4), np.float32), np.zeros(10, np.int64), np.zeros((3, 4), np.float32)
    with pytest.raises(ValueError):
        evaluate.knn_classify(x_train, y_train, x_test, k=k)


def test_knn_shape_errors(no_library):
    with pytest.raises(ValueError):
        evaluate.knn_classify(np.zeros((10, 4), np.float32), np.zeros(10), np.zeros((3, 5), np.float32), k=3)
    with pytest.raises(ValueError):
        evaluate.knn_classify(np.zeros((10, 4), np.float32), np.zeros(9), np.zeros((3, 4), np.float32), k=3)


@pytest.mark.parametrize("k,init_shape", [(3, (4, 8)), (3, (3, 7)), (3, (3,)), (0, None), (65, None), (21, None)])
def test_kmeans_argument_errors(no_library, k, init_shape):
    x = np.zeros((20, 8), np.float32)
    init = None if init_shape is None else np.zeros(init_shape, np.float32)
    with pytest.raises(ValueError):
        evaluate.kmeans(x, k, init=init)
