"""The host side of the silhouette evaluation (data/exp.py:25-62 restated in han_amd.evaluate) against
tests/golden/exp_silhouette_ref.npz, which holds what the reference's own my_Kmeans printed and scikit-learn's
float64 silhouette_samples (tests/golden/gen_silhouette_fixture.py).  No GPU."""
import os

import numpy as np
import pytest

from han_amd import _lib, evaluate
from tests import silhouette_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "exp_silhouette_ref.npz")


@pytest.fixture(scope="module")
def fix():
    return np.load(GOLDEN)


def test_fixture_holds_arrays_only(fix):
    assert sorted(fix.files) == ["labels", "printed", "samples", "seed", "x", "y"]
    assert fix["x"].shape == (300, 16) and fix["x"].dtype == np.float32
    assert all(fix[key].dtype.kind in "fiu" for key in fix.files)
    assert os.path.getsize(GOLDEN) < 64 * 1024


def test_my_kmeans_reproduces_the_numbers_the_reference_printed(fix, capsys):
    pytest.importorskip("sklearn")
    seed = int(fix["seed"])
    three = evaluate.my_Kmeans(fix["x"], fix["y"], k=4, time=10, seed=seed, silhouette=True)
    line = capsys.readouterr().out.strip().splitlines()[-1]
    assert len(three) == 3 and all(isinstance(v, float) for v in three)
    assert np.abs(np.array(three) - fix["printed"]).max() <= 5e-5       # the printed precision
    assert line == "NMI (10 avg): {:.4f} , ARI (10avg): {:.4f}, silhouette(10avg): {:.4f}".format(*fix["printed"])
    two = evaluate.my_Kmeans(fix["x"], fix["y"], k=4, time=10, seed=seed)
    assert capsys.readouterr().out.strip() == "NMI (10 avg): {:.4f} , ARI (10avg): {:.4f}".format(*two)
    assert isinstance(two, tuple) and len(two) == 2 and two == three[:2]


def test_host_samples_and_score_are_scikit_learns(fix):
    pytest.importorskip("sklearn")
    got = evaluate.silhouette_samples(fix["x"], fix["labels"])
    assert isinstance(got, np.ndarray) and got.dtype == np.float64
    assert np.abs(got - fix["samples"]).max() <= 1e-12
    assert abs(evaluate.silhouette_score(fix["x"], fix["labels"]) - fix["samples"].mean()) <= 1e-12
    idx = np.random.RandomState(3).permutation(300)[:120]
    sub = evaluate.silhouette_score(fix["x"], fix["labels"], sample_size=120, seed=3)
    assert abs(sub - evaluate.silhouette_score(fix["x"][idx], fix["labels"][idx])) <= 1e-12
    for bad in (np.zeros(300, dtype=np.int64), np.arange(300)):
        with pytest.raises(ValueError):
            evaluate.silhouette_samples(fix["x"], bad)


def test_numpy_reference_of_the_gpu_tests_is_scikit_learns(fix):
    """tests/silhouette_ref.py (what the GPU tests compare with) against scikit-learn's own float64 values, and its
    bound on the fixture: no undecided row, row bounds far below the values."""
    want = ref.reference(fix["x"], fix["labels"], 4)
    assert np.abs(want["s"] - fix["samples"]).max() <= 1e-12
    assert not want["undecided"].any() and want["bound"].max() < 1e-3
    v, codes = np.array([0, 5, 9, 2, 2, 7]), np.array([0, 0, 1, 1, 2, 2])
    brute = np.abs(v[:, None] - v[None, :]) @ np.eye(3, dtype=np.int64)[codes]
    assert (ref.line_sums(v, codes, 3) == brute).all()


def test_abi_12_declares_the_silhouette_entry_points():
    assert _lib.ABI_VERSION >= 12
    assert {"han_silhouette", "han_silhouette_workspace"} <= set(_lib.SIGNATURES)
    lib = _lib.load()
    assert lib.han_silhouette_workspace(4099, 64, 64) >= 4099 * (4 + 16)      # norms, a and b in double
    assert lib.han_silhouette_workspace(4099, 64, 65) == 0 and lib.han_silhouette_workspace(4099, 513, 4) == 0
    assert lib.han_silhouette_workspace(0, 64, 4) == 0
    # argument checks that return before anything touches the device
    assert lib.han_silhouette(None, 8, None, 10, 8, 1, None, None, None, None, None, 0, None) == -1
    assert lib.han_silhouette(None, 4, None, 10, 8, 2, None, None, None, None, None, 0, None) == -1
    assert lib.han_silhouette(None, 8, None, 10, 8, 65, None, None, None, None, None, 0, None) == -2
    assert lib.han_silhouette(None, 513, None, 10, 513, 2, None, None, None, None, None, 0, None) == -2
